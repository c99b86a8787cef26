//  score-fixed_gpu.cc -- the reference's score-fixed (src/ICM/score-fixed.cc) with its per-string loop replaced by batch calls
//  of the C ABI: all strings are read first, then every model scores all of them in ONE call -- gmg_fixed_score for a
//  fixed-length model (Fixed_Length_ICM_t::Score_Windows), gmg_score_string (frame 1) for the -I negative ICM_t -- and the
//  lines are printed as the reference prints them.  Parse_Command_Line, Read_String and Usage are the reference's own: the file
//  is pulled in whole with its main renamed (integration/Makefile).
//
//  A string the reference would stop at ("too short" under either model) ends the output there: the lines of the strings in
//  front of it, then the reference's message and exit status.

#include "../include/gmg.h"

#include <string>
#include <vector>

#define main score_fixed_reference_main
#include "score-fixed.cc"
#undef main

namespace {

void  Fatal  (const char * who)
  {
   fprintf (stderr, "ERROR:  %s: %s\n", who, gmg_last_error ());
   exit (EXIT_FAILURE);
  }

//  ICM_t::Score_String (s, strlen (s), 1) of every string: the strings as one batch of reads, ONE gmg_score_string call
void  Score_Strings  (const ICM_t & icm, const std::vector <char *> & s, int n, double * out)
  {
   if  (n == 0)
       return;
   std::vector <uint64_t>  off (n + 1, 0);
   for  (int k = 0;  k < n;  k ++)
     off [k + 1] = off [k] + strlen (s [k]);
   std::vector <uint32_t>  packed (gmg_packed_words (off [n]), 0);
   std::vector <gmg_segment>  seg (n);
   for  (int k = 0;  k < n;  k ++)
     {
      gmg_pack_bases (s [k], off [k + 1] - off [k], off [k], packed . data ());
      seg [k] . read = k;
      seg [k] . lo = 0;
      seg [k] . len = uint32_t (off [k + 1] - off [k]);
      seg [k] . orient = GMG_FORWARD;
     }
   gmg_reads  * reads;
   gmg_segments  * segs;
   double  * d_out;
   const gmg_model  * m = icm . Device_Model ();
   if  (gmg_reads_upload (packed . data (), off . data (), n, & reads) != GMG_OK)
       Fatal ("gmg_reads_upload");
   if  (gmg_segments_upload (reads, seg . data (), n, NULL, NULL, & segs) != GMG_OK)
       Fatal ("gmg_segments_upload");
   if  (gmg_device_malloc ((void * *) & d_out, size_t (n) * sizeof (double)) != GMG_OK)
       Fatal ("gmg_device_malloc");
   if  (gmg_score_string (m, reads, segs, 1, d_out, NULL) != GMG_OK)
       Fatal ("gmg_score_string");
   if  (gmg_memcpy_d2h (out, d_out, size_t (n) * sizeof (double), NULL) != GMG_OK || gmg_synchronize (NULL) != GMG_OK)
       Fatal ("gmg_memcpy_d2h");
   gmg_device_free (d_out);
   gmg_segments_free (segs);
   gmg_reads_free (reads);
  }

}  // namespace

int  main
    (int argc, char * argv [])
  {
   Fixed_Length_ICM_t  pos_model;
   ICM_t  neg_icm_model;
   Fixed_Length_ICM_t  neg_fixed_model;
   char  * string = NULL, * tag = NULL;
   long int  string_size = 0, tag_size = 0;
   std::vector <char *>  strings;

   Parse_Command_Line (argc, argv);

   pos_model . read (Pos_Model_Path);
   fprintf (stderr, "pos model  len = %d  special = %d  type = %d\n",
            pos_model . getModelLength (), pos_model . getSpecialPosition (), pos_model . getModelType ());
   if  (Use_Null_Neg_Model)
       fprintf (stderr, "Using null negative model\n");
   else if  (Use_Neg_ICM_Model)
       neg_icm_model . Read (Neg_Model_Path);
     else
       {
        neg_fixed_model . read (Neg_Model_Path);
        fprintf (stderr, "neg model  len = %d  special = %d  type = %d\n",
                 neg_fixed_model . getModelLength (), neg_fixed_model . getSpecialPosition (),
                 neg_fixed_model . getModelType ());
       }
   const bool  neg_fixed = ! Use_Null_Neg_Model && ! Use_Neg_ICM_Model;

   while  (Read_String (stdin, string, string_size, tag, tag_size))
     strings . push_back (strdup (string));

   //  the first string the reference stops at (pos model first, then the negative fixed-length model): scored up to there
   int  n = int (strings . size ());
   std::string  err;
   for  (int k = 0;  k < n;  k ++)
     if  (! pos_model . Check_Window (strings [k], 0, pos_model . getModelLength (), err)
            || (neg_fixed && ! neg_fixed_model . Check_Window (strings [k], 0, neg_fixed_model . getModelLength (), err)))
         {
          n = k;
          break;
         }

   std::vector <double>  pos_score (n), neg_score (n, 0.0);
   if  (n > 0)
       {
        pos_model . Score_Windows (& strings [0], n, 0, pos_model . getModelLength (), pos_score . data ());
        if  (neg_fixed)
            neg_fixed_model . Score_Windows (& strings [0], n, 0, neg_fixed_model . getModelLength (), neg_score . data ());
        else if  (Use_Neg_ICM_Model)
            Score_Strings (neg_icm_model, strings, n, neg_score . data ());
       }

   for  (int k = 0;  k < n;  k ++)
     {
      const int  len = strlen (strings [k]);
      const double  avg_pos_score = pos_score [k] / len, avg_neg_score = neg_score [k] / len;
      if  (Simple_Output)
          printf ("%6d %3d\n", k, pos_score [k] >= neg_score [k] ? 1 : -1);
        else
          printf ("%5d:  %10.4f %9.5f   %10.4f %9.5f   %9.5f\n",
                  k + 1, pos_score [k], avg_pos_score, neg_score [k], avg_neg_score, avg_pos_score - avg_neg_score);
     }
   if  (n < int (strings . size ()))
       {
        fprintf (stderr, "%s\n", err . c_str ());
        exit (EXIT_FAILURE);
       }

   return  0;
  }
