//  gmg_icm_c.cc -- extern "C" wrappers of include/gmg_icm.h over the host ICM_t.

#include "icm.hh"
#include "../../include/gmg_icm.h"
#include "../csrc/gmg_internal.h"   // gmg_set_error

#include <errno.h>
#include <string.h>
#include <new>

using namespace std;

//  The reference keeps this global in src/Common/delcher.cc:20; an application
//  that links its own definition overrides this one.
__attribute__ ((weak)) int  Verbose = 0;

struct gmg_icm
  {
   ICM_Training_t  model;     // an ICM_t with Train_Model; no extra state
   gmg_icm  (int w, int d, int p) : model (w, d, p) {}
  };

extern "C" int  gmg_icm_new  (int w, int d, int p, gmg_icm * * out)
  {
   if  (out == NULL || w < 1 || d < 0 || d > 12 || p < 1)
       return  gmg_set_error (GMG_EINVAL, "gmg_icm_new: bad argument");
   * out = new (nothrow) gmg_icm (w, d, p);
   if  (* out == NULL)
       return  gmg_set_error (GMG_ENOMEM, "gmg_icm_new: out of memory");
   return  GMG_OK;
  }

extern "C" int  gmg_icm_train
    (const char * const * strings, int n_strings, int w, int d, int p, gmg_icm * * out)
  {
   if  (out == NULL || (strings == NULL && n_strings > 0) || n_strings < 0 || w < 1 || d < 0 || d > 12 || p < 1)
       return  gmg_set_error (GMG_EINVAL, "gmg_icm_train: bad argument");
   gmg_icm  * h = new (nothrow) gmg_icm (w, d, p);
   if  (h == NULL)
       return  gmg_set_error (GMG_ENOMEM, "gmg_icm_train: out of memory");
   string  err;
   if  (! h -> model . Try_Train_Model (strings, n_strings, err))
       {
        delete  h;
        return  gmg_set_error (GMG_EHIP, "%s", err . c_str ());
       }
   * out = h;
   return  GMG_OK;
  }

extern "C" int  gmg_icm_train_reads
    (const gmg_reads * strings, int w, int d, int p, gmg_icm * * out)
  {
   if  (out == NULL || strings == NULL || w < 1 || d < 0 || d > 12 || p < 1)
       return  gmg_set_error (GMG_EINVAL, "gmg_icm_train_reads: bad argument");
   gmg_icm  * h = new (nothrow) gmg_icm (w, d, p);
   if  (h == NULL)
       return  gmg_set_error (GMG_ENOMEM, "gmg_icm_train_reads: out of memory");
   string  err;
   if  (! h -> model . Try_Train_Reads (strings, err))
       {
        delete  h;
        return  gmg_set_error (GMG_EHIP, "%s", err . c_str ());
       }
   * out = h;
   return  GMG_OK;
  }

extern "C" int  gmg_icm_open  (const char * path, gmg_icm * * out)
  {
   if  (path == NULL || out == NULL)
       return  gmg_set_error (GMG_EINVAL, "gmg_icm_open: NULL argument");
   FILE  * fp = fopen (path, "rb");
   if  (fp == NULL)
       return  gmg_set_error (GMG_EINVAL, "ERROR:  Could not open file  %s  errno = %d", path, errno);
   gmg_icm  * h = new (nothrow) gmg_icm (1, 0, 1);
   if  (h == NULL)
       {
        fclose (fp);
        return  gmg_set_error (GMG_ENOMEM, "gmg_icm_open: out of memory");
       }
   string  err;
   bool  ok = h -> model . Try_Input (fp, err);
   fclose (fp);
   if  (! ok)
       {
        delete  h;
        return  gmg_set_error (GMG_EBADMODEL, "%s", err . c_str ());
       }
   * out = h;
   return  GMG_OK;
  }

extern "C" int  gmg_icm_build_indep
    (gmg_icm * icm, double gc_frac, const char * const * stop_codon, int n_stops)
  {
   if  (icm == NULL || (n_stops > 0 && stop_codon == NULL))
       return  gmg_set_error (GMG_EINVAL, "gmg_icm_build_indep: NULL argument");
   ICM_t  & m = icm -> model;
   if  (m . Get_Model_Len () != 3 || m . Get_Model_Depth () != 2 || m . Get_Periodicity () != 3
          || m . Get_Num_Nodes () != 21)
       return  gmg_set_error (GMG_EBADMODEL, "ERROR:  Incompatible ICM_Training_t for Build_Indep_WO_Stops");
   vector <const char *>  stops;
   for  (int i = 0;  i < n_stops;  i ++)
     {
      if  (stop_codon [i] == NULL || strlen (stop_codon [i]) < 3)
          return  gmg_set_error (GMG_EINVAL, "gmg_icm_build_indep: stop codon %d is not 3 letters", i);
      stops . push_back (stop_codon [i]);
     }
   m . Build_Indep_WO_Stops (gc_frac, stops);
   return  GMG_OK;
  }

extern "C" int  gmg_icm_write  (gmg_icm * icm, const char * path)
  {
   if  (icm == NULL || path == NULL)
       return  gmg_set_error (GMG_EINVAL, "gmg_icm_write: NULL argument");
   FILE  * fp = fopen (path, "wb");
   if  (fp == NULL)
       return  gmg_set_error (GMG_EINVAL, "ERROR:  Could not open file  %s  errno = %d", path, errno);
   icm -> model . Output (fp, true);
   if  (fclose (fp) != 0)
       return  gmg_set_error (GMG_EINVAL, "gmg_icm_write: write to %s failed", path);
   return  GMG_OK;
  }

extern "C" int  gmg_icm_free  (gmg_icm * icm)
  {
   delete  icm;
   return  GMG_OK;
  }

extern "C" int  gmg_icm_params
    (const gmg_icm * icm, int * w, int * d, int * p, int * n)
  {
   if  (icm == NULL)
       return  gmg_set_error (GMG_EINVAL, "gmg_icm_params: NULL model");
   ICM_t  & m = const_cast <ICM_Training_t &> (icm -> model);
   if  (w)  * w = m . Get_Model_Len ();
   if  (d)  * d = m . Get_Model_Depth ();
   if  (p)  * p = m . Get_Periodicity ();
   if  (n)  * n = m . Get_Num_Nodes ();
   return  GMG_OK;
  }

extern "C" int  gmg_icm_tables  (const gmg_icm * icm, int16_t * mip, float * prob4)
  {
   if  (icm == NULL || mip == NULL || prob4 == NULL)
       return  gmg_set_error (GMG_EINVAL, "gmg_icm_tables: NULL argument");
   vector <short>  m;
   vector <float>  p;
   icm -> model . Export_Tables (m, p);
   memcpy (mip, m . data (), m . size () * sizeof (short));
   memcpy (prob4, p . data (), p . size () * sizeof (float));
   return  GMG_OK;
  }

extern "C" int  gmg_icm_device_model  (const gmg_icm * icm, const gmg_model * * out)
  {
   if  (icm == NULL || out == NULL)
       return  gmg_set_error (GMG_EINVAL, "gmg_icm_device_model: NULL argument");
   //  ICM_t::Device_Model exits on failure (reference convention); check the one likely cause first
   //  so that this C entry point returns a status instead
   if  (gmg_device_count () <= 0)
       return  gmg_set_error (GMG_ENODEV, "gmg_icm_device_model: no HIP device; there is no CPU fallback");
   * out = icm -> model . Device_Model ();
   return  GMG_OK;
  }


//  tests (tests/test_gpu_threads.py; not declared in include/*.h): ICM_t::Score_String of one string -- the host class's
//  one-call-one-launch path, which makes the calling thread's staging (Thread_Staging, icm.cc) at the thread's first call.
//  A string of length 0 scores 0.0 as in the reference (src/ICM/icm.cc:864-903): no launch, and no staging is made.
extern "C" int  gmg_debug_icm_score_string  (const gmg_icm * icm, const char * s, int len, int frame, double * out)
  {
   int  periodicity = 0;
   if  (icm == NULL || s == NULL || out == NULL || len < 0 || frame < 0
          || gmg_icm_params (icm, NULL, NULL, & periodicity, NULL) != GMG_OK || frame >= periodicity)
       return  gmg_set_error (GMG_EINVAL, "gmg_debug_icm_score_string: bad argument");
   if  (gmg_device_count () <= 0)
       return  gmg_set_error (GMG_ENODEV, "gmg_debug_icm_score_string: no HIP device; there is no CPU fallback");
   * out = icm -> model . Score_String (s, len, frame);
   return  GMG_OK;
  }


// ---------------------------------------------------------------------------
// fixed-length ICMs
// ---------------------------------------------------------------------------

struct gmg_fixed_icm
  {
   Fixed_Length_ICM_t  scorer;
   Fixed_Length_ICM_Training_t  * trained;     // NULL for a model that was read
   gmg_fixed_icm  ()  : trained (NULL)  {}
   ~ gmg_fixed_icm  ()  { delete  trained; }
  };

//  the scorer of a trained model: its binary bytes read back through the same path as a file (Try_Input)
static bool  Load_Trained  (gmg_fixed_icm * h, string & err)
  {
   char  * buf = NULL;
   size_t  len = 0;
   FILE  * mem = open_memstream (& buf, & len);
   if  (mem == NULL)
       { err = "gmg_fixed_icm_train: open_memstream failed";  return  false; }
   h -> trained -> Output (mem, true);
   fclose (mem);
   FILE  * in = fmemopen (buf, len, "rb");
   bool  ok = (in != NULL) && h -> scorer . Try_Input (in, err);
   if  (in != NULL)
       fclose (in);
   free (buf);
   return  ok;
  }

extern "C" int  gmg_fixed_icm_read  (const char * path, gmg_fixed_icm * * out)
  {
   if  (path == NULL || out == NULL)
       return  gmg_set_error (GMG_EINVAL, "gmg_fixed_icm_read: NULL argument");
   gmg_fixed_icm  * h = new (nothrow) gmg_fixed_icm ();
   if  (h == NULL)
       return  gmg_set_error (GMG_ENOMEM, "gmg_fixed_icm_read: out of memory");
   string  err;
   if  (! h -> scorer . Try_Read (path, err))
       {
        delete  h;
        return  gmg_set_error (GMG_EBADMODEL, "%s", err . c_str ());
       }
   * out = h;
   return  GMG_OK;
  }

extern "C" int  gmg_fixed_icm_train
    (const char * const * strings, int n, int max_depth, int special, const int * perm, gmg_fixed_icm * * out)
  {
   if  (out == NULL || strings == NULL || n < 1 || max_depth < 0 || max_depth > 12)
       return  gmg_set_error (GMG_EINVAL, "gmg_fixed_icm_train: bad argument");
   const int  len = int (strlen (strings [0]));
   for  (int i = 0;  i < n;  i ++)
     if  (strings [i] == NULL || int (strlen (strings [i])) != len)
         return  gmg_set_error (GMG_EINVAL, "gmg_fixed_icm_train: string #%d has a length different from string #0 length = %d", i, len);
   if  (len < 1 || len > 32)
       return  gmg_set_error (GMG_EBADMODEL, "gmg_fixed_icm_train: length %d outside 1 .. 32", len);
   if  (perm != NULL)
     {
      vector <bool>  seen (len, false);
      for  (int i = 0;  i < len;  i ++)
        {
         if  (perm [i] < 0 || perm [i] >= len || seen [perm [i]])
             return  gmg_set_error (GMG_EBADMODEL, "gmg_fixed_icm_train: the permutation is not a bijection of 0..%d", len - 1);
         seen [perm [i]] = true;
        }
     }
   //  Train_Model permutes its strings in place: train on copies
   vector <string>  copies (strings, strings + n);
   vector <char *>  data (n);
   for  (int i = 0;  i < n;  i ++)
     data [i] = & copies [i] [0];
   gmg_fixed_icm  * h = new (nothrow) gmg_fixed_icm ();
   if  (h == NULL)
       return  gmg_set_error (GMG_ENOMEM, "gmg_fixed_icm_train: out of memory");
   h -> trained = new Fixed_Length_ICM_Training_t (len, max_depth, special, const_cast <int *> (perm));
   string  err;
   if  (! h -> trained -> Try_Train_Model (data, err) || ! Load_Trained (h, err))
       {
        delete  h;
        return  gmg_set_error (GMG_EHIP, "%s", err . c_str ());
       }
   * out = h;
   return  GMG_OK;
  }

extern "C" int  gmg_fixed_icm_write  (gmg_fixed_icm * icm, const char * path, int binary)
  {
   if  (icm == NULL || path == NULL)
       return  gmg_set_error (GMG_EINVAL, "gmg_fixed_icm_write: NULL argument");
   if  (icm -> trained == NULL)
       return  gmg_set_error (GMG_EINVAL, "gmg_fixed_icm_write: only a model trained here can be written (Fixed_Length_ICM_t has no Output)");
   FILE  * fp = fopen (path, "wb");
   if  (fp == NULL)
       return  gmg_set_error (GMG_EINVAL, "ERROR:  Could not open file  %s  errno = %d", path, errno);
   icm -> trained -> Output (fp, binary != 0);
   if  (fclose (fp) != 0)
       return  gmg_set_error (GMG_EINVAL, "gmg_fixed_icm_write: write to %s failed", path);
   return  GMG_OK;
  }

extern "C" int  gmg_fixed_icm_params
    (const gmg_fixed_icm * icm, int * length, int * max_depth, int * special, int * type, int * perm)
  {
   if  (icm == NULL)
       return  gmg_set_error (GMG_EINVAL, "gmg_fixed_icm_params: NULL model");
   Fixed_Length_ICM_t  & m = const_cast <Fixed_Length_ICM_t &> (icm -> scorer);
   if  (length)  * length = m . getModelLength ();
   if  (max_depth)  * max_depth = m . Get_Max_Depth ();
   if  (special)  * special = m . getSpecialPosition ();
   if  (type)  * type = m . getModelType ();
   if  (perm && m . Get_Permutation () != NULL)
       memcpy (perm, m . Get_Permutation (), m . getModelLength () * sizeof (int));
   return  GMG_OK;
  }

extern "C" int  gmg_fixed_icm_score
    (gmg_fixed_icm * icm, const char * const * strings, int n, int lo, int hi, double * out)
  {
   if  (icm == NULL || (n > 0 && (strings == NULL || out == NULL)) || n < 0)
       return  gmg_set_error (GMG_EINVAL, "gmg_fixed_icm_score: bad argument");
   for  (int k = 0;  k < n;  k ++)
     if  (strings [k] == NULL)
         return  gmg_set_error (GMG_EINVAL, "gmg_fixed_icm_score: string %d is NULL", k);
   //  the reference's checks first (host only), so that their messages do not depend on a device
   string  err;
   if  (lo < 0 || icm -> scorer . getModelLength () < hi || hi < lo)
       return  gmg_set_error (GMG_EINVAL, "ERROR:  Bad range  lo = %d  hi = %d  in subrange_score", lo, hi);
   for  (int k = 0;  k < n;  k ++)
     if  (! icm -> scorer . Check_Window (strings [k], lo, hi, err))
         return  gmg_set_error (err . find ("too short") != string :: npos ? GMG_ERANGE : GMG_EINVAL, "%s", err . c_str ());
   if  (gmg_device_count () <= 0)
       return  gmg_set_error (GMG_ENODEV, "gmg_fixed_icm_score: no HIP device; there is no CPU fallback");
   if  (! icm -> scorer . Try_Score_Windows (strings, n, lo, hi, out, err))
       return  gmg_set_error (err . find ("too short") != string :: npos ? GMG_ERANGE : GMG_EINVAL, "%s", err . c_str ());
   return  GMG_OK;
  }

extern "C" int  gmg_fixed_icm_device_model  (gmg_fixed_icm * icm, const gmg_fixed_model * * out)
  {
   if  (icm == NULL || out == NULL)
       return  gmg_set_error (GMG_EINVAL, "gmg_fixed_icm_device_model: NULL argument");
   if  (gmg_device_count () <= 0)
       return  gmg_set_error (GMG_ENODEV, "gmg_fixed_icm_device_model: no HIP device; there is no CPU fallback");
   * out = icm -> scorer . Device_Model ();
   return  GMG_OK;
  }

extern "C" int  gmg_fixed_icm_free  (gmg_fixed_icm * icm)
  {
   delete  icm;
   return  GMG_OK;
  }
