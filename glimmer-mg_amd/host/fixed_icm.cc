//  fixed_icm.cc -- host side of the fixed-length ICMs (see icm.hh): Fixed_Length_ICM_t, Fixed_Length_ICM_Training_t,
//  Permute_Data and Permute_String (reference: src/ICM/icm.hh:216-302, src/ICM/icm.cc:1466-1836,1958-2004).
//
//  Model I/O, the checks and the permutation of training strings are host code, as in the reference.  Scoring is one
//  gmg_fixed_score call (include/gmg.h) per Score_Window / subrange_score, or per batch; training is the device trainer of
//  ICM_Training_t, once per sub-model.

#include "icm.hh"
#include "icm_internal.hh"
#include "../../include/gmg.h"

#include <errno.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

using namespace std;
using gmg_host :: Device_Fatal;
using gmg_host :: Ensure_Device;
using gmg_host :: Thread_Staging;

namespace {

const int  MAX_FIXED_LEN = 32;     // GMG_MAX_MODEL_LEN: the window's 2-bit codes fit one 64-bit register

bool  Is_Bijection  (const int * perm, int n)
  {
   vector <bool>  seen (n, false);
   for  (int i = 0;  i < n;  i ++)
     {
      if  (perm [i] < 0 || perm [i] >= n || seen [perm [i]])
          return  false;
      seen [perm [i]] = true;
     }
   return  true;
  }

//  the constructors' copy of a caller's permutation (NULL stays NULL); a permutation that is not one is refused
int  * Copy_Permutation  (const int * perm, int len, const char * who)
  {
   if  (perm == NULL)
       return  NULL;
   if  (len < 1 || ! Is_Bijection (perm, len))
       {
        fprintf (stderr, "ERROR:  %s:  the permutation is not a bijection of 0..%d\n", who, len - 1);
        exit (EXIT_FAILURE);
       }
   int  * p = new int [len];
   memcpy (p, perm, len * sizeof (int));
   return  p;
  }

string  Format  (const char * fmt, ...)  __attribute__ ((format (printf, 1, 2)));
string  Format  (const char * fmt, ...)
  {
   char  buf [512];
   va_list  ap;
   va_start (ap, fmt);
   vsnprintf (buf, sizeof buf, fmt, ap);
   va_end (ap);
   return  string (buf);
  }

}  // namespace


// ---------------------------------------------------------------------------
// Permute_Data / Permute_String (src/ICM/icm.cc:1958-2004)
// ---------------------------------------------------------------------------

//  every string rearranged by  perm , all with the length of the first one
void  Permute_Data  (vector <char *> & data, int * perm)
  {
   if  (data . empty ())
       return;
   int  len = strlen (data [0]);
   for  (size_t i = 0;  i < data . size ();  i ++)
     Permute_String (data [i], perm, len);
  }

//  s [i] = old s [perm [i]] for i < n.  The copy back is strncpy, as in the reference: a '\0' that lands at position j clears
//  positions j .. n-1 (the "too short" checks of Score_Window / subrange_score depend on it).
void  Permute_String  (char * s, int * perm, int n)
  {
   vector <char>  buff (n > 0 ? n : 1);
   for  (int i = 0;  i < n;  i ++)
     buff [i] = s [perm [i]];
   strncpy (s, buff . data (), n);
  }


// ---------------------------------------------------------------------------
// Fixed_Length_ICM_t
// ---------------------------------------------------------------------------

//  src/ICM/icm.cc:1466-1487
Fixed_Length_ICM_t :: Fixed_Length_ICM_t  (int len, int sp, int * perm, ICM_Model_t mt)
  {
   length = len;
   max_depth = 0;
   permutation = Copy_Permutation (perm, len, "Fixed_Length_ICM_t");
   special_position = sp;
   model_type = mt;
   dev_fixed = NULL;
  }

Fixed_Length_ICM_t :: ~ Fixed_Length_ICM_t  ()
  {
   Clear ();
   delete [] permutation;
  }

void  Fixed_Length_ICM_t :: Clear  (void)
  {
   if  (gmg_host :: Mirror_Load (dev_fixed) != NULL)        //  (a model without a mirror never touches the lock)
     {
      std :: lock_guard <std :: mutex>  lock (gmg_host :: Mirror_Mutex ());      //  (not around the sub-models: they take it themselves)
      if  (dev_fixed != NULL)
          {
           gmg_fixed_model_free (dev_fixed);
           gmg_host :: Mirror_Store (dev_fixed, (gmg_fixed_model *) NULL);
          }
     }
   for  (size_t i = 0;  i < sub_model . size ();  i ++)
     delete  sub_model [i];
   sub_model . clear ();
  }

//  src/ICM/icm.cc:1502-1559: the 150-byte text line, six int32 {version, 150, length, max_depth, special, type}, the
//  permutation (length int32), then  length  ICM_t models back to back, each read by ICM_t::Input (which stops at the model's
//  end marker: exactly its own bytes)
bool  Fixed_Length_ICM_t :: Try_Input  (FILE * fp, string & err)
  {
   char  line [ID_STRING_LEN];
   int  param [NUM_FIXED_LENGTH_PARAMS];

   Clear ();
   if  (fread (line, sizeof (char), ID_STRING_LEN, fp) != size_t (ID_STRING_LEN)
          || fread (param, sizeof (int), NUM_FIXED_LENGTH_PARAMS, fp) != NUM_FIXED_LENGTH_PARAMS)
       { err = "ERROR reading file";  return  false; }
   if  (param [0] != ICM_VERSION_ID)
       { err = Format ("Bad ICM version = %d  should be %d", param [0], ICM_VERSION_ID);  return  false; }
   if  (param [1] != ID_STRING_LEN)
       { err = Format ("Bad ID_STRING_LEN = %d  should be %d", param [1], ID_STRING_LEN);  return  false; }
   if  (param [2] < 1 || param [2] > MAX_FIXED_LEN)
       { err = Format ("ERROR:  Fixed-length model length = %d  must be 1 .. %d", param [2], MAX_FIXED_LEN);  return  false; }

   vector <int>  perm (param [2]);
   if  (fread (perm . data (), sizeof (int), param [2], fp) != size_t (param [2]))
       { err = "ERROR reading file";  return  false; }
   if  (! Is_Bijection (perm . data (), param [2]))
       { err = Format ("ERROR:  the permutation of the fixed-length model is not a bijection of 0..%d", param [2] - 1);  return  false; }

   length = param [2];
   max_depth = param [3];
   special_position = param [4];
   model_type = ICM_Model_t (param [5]);
   delete [] permutation;
   permutation = new int [length];
   memcpy (permutation, perm . data (), length * sizeof (int));

   for  (int i = 0;  i < length;  i ++)
     {
      ICM_t  * p = new ICM_t (1, 0, 1);
      sub_model . push_back (p);
      if  (! p -> Try_Input (fp, err))
          return  false;
      if  (p -> Get_Model_Len () != i + 1 || p -> Get_Periodicity () != 1)
          {
           err = Format ("ERROR:  sub-model %d of the fixed-length model has model_len = %d  periodicity = %d"
                         "  (should be %d and 1)", i, p -> Get_Model_Len (), p -> Get_Periodicity (), i + 1);
           return  false;
          }
     }
   return  true;
  }

bool  Fixed_Length_ICM_t :: Try_Read  (const char * path, string & err)
  {
   FILE  * fp = fopen (path, "r");
   if  (fp == NULL)
       {
        err = Format ("ERROR:  Could not open file  %s\n  errno = %d", path, errno);
        return  false;
       }
   bool  ok = Try_Input (fp, err);
   fclose (fp);
   if  (! ok && err == "ERROR reading file")
       err = Format ("ERROR reading file \"%s\"", path);
   return  ok;
  }

void  Fixed_Length_ICM_t :: read  (const char * path)
  {
   string  err;
   if  (! Try_Read (path, err))
       {
        fprintf (stderr, "%s\n", err . c_str ());
        exit (EXIT_FAILURE);
       }
  }

const gmg_fixed_model *  Fixed_Length_ICM_t :: Device_Model  (void)  const
  {
   //  the first use may come from several threads at once: one of them uploads (icm_internal.hh)
   gmg_fixed_model  * m = gmg_host :: Mirror_Load (dev_fixed);
   if  (m != NULL)
       return  m;
   //  nothing reaches exit () with the lock held (ICM_t::Device_Model says why)
   if  (sub_model . empty ())
       {
        fprintf (stderr, "ERROR:  Fixed_Length_ICM_t used before read\n");
        exit (EXIT_FAILURE);
       }
   Ensure_Device ();
   bool  failed = false;
   std :: unique_lock <std :: mutex>  lock (gmg_host :: Mirror_Mutex ());
   m = dev_fixed;
   if  (m == NULL)
       {
        vector < vector <short> >  mip (length);
        vector < vector <float> >  prob (length);
        vector <const int16_t *>  mp (length);
        vector <const float *>  pp (length);
        vector <int>  depth (length), nodes (length);
        for  (int i = 0;  i < length;  i ++)
          {
           sub_model [i] -> Export_Tables (mip [i], prob [i]);
           mp [i] = mip [i] . data ();
           pp [i] = prob [i] . data ();
           depth [i] = sub_model [i] -> Get_Model_Depth ();
           nodes [i] = sub_model [i] -> Get_Num_Nodes ();
          }
        failed = gmg_fixed_model_upload (length, permutation, mp . data (), pp . data (), depth . data (), nodes . data (),
                                         & m) != GMG_OK;
        if  (! failed)
            gmg_host :: Mirror_Store (dev_fixed, m);
       }
   lock . unlock ();
   if  (failed)
       Device_Fatal ("gmg_fixed_model_upload");
   return  m;
  }

//  The reference's checks on one window (src/ICM/icm.cc:1575-1600, 1617-1642): strncpy (buff, w, length), Permute_String,
//  then "too short" at the first i in [lo, hi) with buff [i] == '\0'.  (strncpy pads with '\0' and Permute_String's own
//  strncpy clears everything behind the first '\0' that lands in the permuted window, so that is the first '\0' of the
//  permuted window, when it is below hi.)  The message shows the permuted window up to that '\0'.
bool  Fixed_Length_ICM_t :: Check_Window  (const char * w, int lo, int hi, string & err)  const
  {
   if  (sub_model . empty () || permutation == NULL)
       {
        err = "ERROR:  Fixed_Length_ICM_t used before read";
        return  false;
       }
   if  (lo >= hi)
       return  true;
   int  n = 0;
   while  (n < length && w [n] != '\0')
     n ++;
   if  (n == length)
       return  true;
   int  first = length;
   for  (int i = 0;  i < length;  i ++)
     if  (permutation [i] >= n)
         { first = i;  break; }
   if  (first >= hi)
       return  true;
   string  shown;
   for  (int i = 0;  i < first;  i ++)
     shown += w [permutation [i]];
   err = "ERROR:  String \"" + shown + "\" too short in Score_Window";
   return  false;
  }

//  src/ICM/icm.cc:1563-1602: ONE device call (the thread's one-string staging, gmg_fixed_score over all L sub-models)
double  Fixed_Length_ICM_t :: Score_Window  (char * w)
  {
   return  subrange_score (w, 0, length);
  }

//  src/ICM/icm.cc:1606-1645
double  Fixed_Length_ICM_t :: subrange_score  (char * w, int lo, int hi)
  {
   string  err;
   if  (lo < 0 || length < hi || hi < lo)
       {
        fprintf (stderr, "ERROR:  Bad range  lo = %d  hi = %d  in subrange_score\n", lo, hi);
        exit (EXIT_FAILURE);
       }
   if  (! Check_Window (w, lo, hi, err))
       {
        fprintf (stderr, "%s\n", err . c_str ());
        exit (EXIT_FAILURE);
       }
   if  (lo == hi)
       return  0.0;
   const gmg_fixed_model  * m = Device_Model ();
   const gmg_reads  * reads;
   const gmg_segments  * segs;
   double  * d_out, result;
   gmg_single  * stage = Thread_Staging ();
   //  the window is complete below hi; characters at or past a '\0' are never scored (Check_Window), so staging the
   //  first  length  bytes as they are ('\0' packs as a base like any other character) gives the same sum
   char  buff [MAX_FIXED_LEN];
   strncpy (buff, w, length);
   if  (gmg_single_stage (stage, buff, (uint64_t) length, GMG_FORWARD, & reads, & segs, & d_out) != GMG_OK)
       Device_Fatal ("Fixed_Length_ICM_t device staging");
   if  (gmg_fixed_score (m, reads, segs, lo, hi, d_out, NULL) != GMG_OK)
       Device_Fatal ("gmg_fixed_score");
   if  (gmg_single_fetch (stage, & result, 1) != GMG_OK)
       Device_Fatal ("Fixed_Length_ICM_t result copy");
   return  result;
  }

bool  Fixed_Length_ICM_t :: Try_Score_Windows
    (const char * const * strings, int n, int lo, int hi, double * out, string & err)
  {
   if  (lo < 0 || length < hi || hi < lo)
       {
        err = Format ("ERROR:  Bad range  lo = %d  hi = %d  in subrange_score", lo, hi);
        return  false;
       }
   if  (n <= 0)
       return  true;
   for  (int k = 0;  k < n;  k ++)
     if  (! Check_Window (strings [k], lo, hi, err))
         return  false;
   if  (lo == hi)
       {
        for  (int k = 0;  k < n;  k ++)
          out [k] = 0.0;
        return  true;
       }
   const gmg_fixed_model  * m = Device_Model ();

   //  the windows back to back as ONE read (length bases each, strncpy's padding included), a segment per window
   const uint64_t  total = uint64_t (n) * length;
   vector <char>  text (total);
   for  (int k = 0;  k < n;  k ++)
     strncpy (text . data () + uint64_t (k) * length, strings [k], length);
   vector <uint32_t>  packed (gmg_packed_words (total), 0);
   uint64_t  off [2] = {0, total};
   vector <gmg_segment>  seg (n);
   for  (int k = 0;  k < n;  k ++)
     {
      seg [k] . read = 0;
      seg [k] . lo = uint32_t (uint64_t (k) * length);
      seg [k] . len = uint32_t (length);
      seg [k] . orient = GMG_FORWARD;
     }
   gmg_reads  * reads = NULL;
   gmg_segments  * segs = NULL;
   double  * d_out = NULL;
   bool  ok = total <= 0xffffffffull
                && gmg_pack_bases (text . data (), total, 0, packed . data ()) == GMG_OK
                && gmg_reads_upload (packed . data (), off, 1, & reads) == GMG_OK
                && gmg_segments_upload (reads, seg . data (), n, NULL, NULL, & segs) == GMG_OK
                && gmg_device_malloc ((void * *) & d_out, size_t (n) * sizeof (double)) == GMG_OK
                && gmg_fixed_score (m, reads, segs, lo, hi, d_out, NULL) == GMG_OK
                && gmg_memcpy_d2h (out, d_out, size_t (n) * sizeof (double), NULL) == GMG_OK
                && gmg_synchronize (NULL) == GMG_OK;
   if  (! ok)
       err = total > 0xffffffffull ? string ("Score_Windows: more than 2^32 bases in one call")
                                   : string ("Score_Windows: ") + gmg_last_error ();
   if  (d_out != NULL)
       gmg_device_free (d_out);
   if  (segs != NULL)
       gmg_segments_free (segs);
   if  (reads != NULL)
       gmg_reads_free (reads);
   return  ok;
  }

void  Fixed_Length_ICM_t :: Score_Windows
    (const char * const * strings, int n, int lo, int hi, double * out)
  {
   string  err;
   Ensure_Device ();
   if  (! Try_Score_Windows (strings, n, lo, hi, out, err))
       {
        fprintf (stderr, "%s\n", err . c_str ());
        exit (EXIT_FAILURE);
       }
  }


// ---------------------------------------------------------------------------
// Fixed_Length_ICM_Training_t
// ---------------------------------------------------------------------------

//  src/ICM/icm.cc:1649-1668
Fixed_Length_ICM_Training_t :: Fixed_Length_ICM_Training_t
    (int len, int md, int sp, int * perm, ICM_Model_t mt)
  {
   if  (len < 1 || len > MAX_FIXED_LEN)
       {
        fprintf (stderr, "ERROR:  Fixed-length model length = %d  must be 1 .. %d\n", len, MAX_FIXED_LEN);
        exit (EXIT_FAILURE);
       }
   length = len;
   max_depth = md;
   special_position = sp;
   permutation = Copy_Permutation (perm, len, "Fixed_Length_ICM_Training_t");
   model_type = mt;
  }

Fixed_Length_ICM_Training_t :: ~ Fixed_Length_ICM_Training_t  ()
  {
   delete [] permutation;
   for  (size_t i = 0;  i < sub_model . size ();  i ++)
     delete  sub_model [i];
  }

//  src/ICM/icm.cc:1691-1707
void  Fixed_Length_ICM_Training_t :: Output  (FILE * fp, bool binary_form)
  {
   Write_Header (fp, binary_form);
   for  (size_t i = 0;  i < sub_model . size ();  i ++)
     sub_model [i] -> Output (fp, binary_form);
  }

bool  Fixed_Length_ICM_Training_t :: Try_Train_Model  (vector <char *> & data, string & err)
  {
   const int  string_ct = int (data . size ());

   if  (permutation != NULL)
       Permute_Data (data, permutation);

   for  (size_t i = 0;  i < sub_model . size ();  i ++)
     delete  sub_model [i];
   sub_model . clear ();

   //  the length-i prefixes of every (permuted) string, for i = 1 .. length
   vector <char>  store (size_t (string_ct) * (length + 1));
   vector <char *>  sub_data (string_ct);
   for  (int j = 0;  j < string_ct;  j ++)
     sub_data [j] = store . data () + size_t (j) * (length + 1);

   for  (int i = 1;  i <= length;  i ++)
     {
      for  (int j = 0;  j < string_ct;  j ++)
        {
         strncpy (sub_data [j], data [j], i);
         sub_data [j] [i] = '\0';
        }
      const int  depth = (i - 1 < max_depth ? i - 1 : max_depth);
      ICM_Training_t  * mp = new ICM_Training_t (i, depth, 1);
      sub_model . push_back (mp);
      if  (! mp -> Try_Train_Model (string_ct ? sub_data . data () : NULL, string_ct, err))
          return  false;
     }
   return  true;
  }

//  src/ICM/icm.cc:1711-1759
void  Fixed_Length_ICM_Training_t :: Train_Model  (vector <char *> & data)
  {
   string  err;
   if  (! Try_Train_Model (data, err))
       {
        fprintf (stderr, "ERROR:  %s\n", err . c_str ());
        exit (EXIT_FAILURE);
       }
  }

//  src/ICM/icm.cc:1763-1836: the text form is one line; the binary form is that line (with a leading '>') in a zero-filled
//  150-byte field, the six parameters and the permutation (the identity when there is none)
void  Fixed_Length_ICM_Training_t :: Write_Header  (FILE * fp, bool binary_form)
  {
   string  line = Format ("ver=%.2f  len=%d  depth=%d  special=%d  type=%d",
                          ICM_VERSION_ID / 100.0, length, max_depth, special_position, int (model_type));
   for  (int i = 0;  i < length;  i ++)
     line += Format (i == 0 ? "  %d" : ",%d", permutation == NULL ? i : permutation [i]);
   line += "\n";

   if  (! binary_form)
       {
        fputs (line . c_str (), fp);
        return;
       }

   char  field [ID_STRING_LEN];
   memset (field, 0, sizeof field);
   line = ">" + line;
   if  (int (line . size ()) >= ID_STRING_LEN)
       {
        fprintf (stderr, "ERROR:  fixed-length model header of %d characters does not fit %d bytes\n",
                 int (line . size ()), ID_STRING_LEN);
        exit (EXIT_FAILURE);
       }
   memcpy (field, line . data (), line . size ());
   fwrite (field, sizeof (char), ID_STRING_LEN, fp);

   int  param [NUM_FIXED_LENGTH_PARAMS] = {ICM_VERSION_ID, ID_STRING_LEN, length, max_depth, special_position,
                                           int (model_type)};
   fwrite (param, sizeof (int), NUM_FIXED_LENGTH_PARAMS, fp);
   vector <int>  perm (length);
   for  (int i = 0;  i < length;  i ++)
     perm [i] = (permutation == NULL ? i : permutation [i]);
   fwrite (perm . data (), sizeof (int), length, fp);
  }
