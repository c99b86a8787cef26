//  build-icm_gpu.cc -- `extract <opts> seq coords | build-icm <opts> out.icm` in one process, without the text in between: the
//  sequence file is ingested on the device (gmg_fasta_ingest), the coordinate lines become regions (gmg_extract_plan), the regions
//  a batch of training strings in HBM (gmg_reads_extract, back to front under -r) and the model is trained from that batch
//  (ICM_Training_t::Try_Train_Reads).  Parse_Command_Line, Usage and the option variables are the reference's own: build-icm.cc is
//  pulled in whole with its main renamed (integration/Makefile).
//
//      build-icm_gpu [build-icm options] --extract [-d] [-l N] [-s] [-t] [-w] [--multi] <sequence-file> <coords> <output.icm>
//      build-icm_gpu [build-icm options] --list <jobs>     one "<extract options> <sequence-file> <coords> <output.icm>" per line
//      build-icm_gpu [build-icm options] <output.icm> < training.fa                      (build-icm_dropin's behaviour)
//
//  extract reads the FIRST record of the sequence file.  With --multi the coordinate lines are multi-extract's, "<id> <tag> <start>
//  <end> [dir]": every record whose first header token equals the tag takes part, a tag without a record is skipped.  --list runs
//  any number of jobs under one gmg_init (GMG_DEVICE selects the GPU); --timing prints every job's stages on stderr.
//
//  Two differences from the reference's pipe, both refusals: -F (build-icm compares the raw letters of a string with the stop
//  codons; the batch holds 2-bit codes) exits with status 2 when combined with --extract / --list, and a coordinate line that
//  asks for more bases than its sequence holds (extract walks round the circle again) ends the run with status 1 and the line.

#include "../include/gmg.h"

#include <time.h>
#include <map>
#include <string>
#include <vector>

#define main build_icm_reference_main
#include "build-icm.cc"
#undef main

namespace {

struct  Job_t
  {
   int  flags;
   long int  min_len;
   bool  multi;
   std::string  seq_path, coord_path, out_path;
   Job_t  ()  : flags (0), min_len (0), multi (false)  {}
  };

//  wall time of a job's stages (--timing)
struct  Laps_t
  {
   double  ms [5], prev;
   static double  Now  ()
     {
      struct timespec  ts;
      clock_gettime (CLOCK_MONOTONIC, & ts);
      return  1e3 * ts . tv_sec + 1e-6 * ts . tv_nsec;
     }
   Laps_t  ()
     {
      for  (int k = 0;  k < 5;  k ++)
        ms [k] = 0.0;
      prev = Now ();
     }
   void  Lap  (int k)
     {
      const double  t = Now ();
      ms [k] += t - prev;
      prev = t;
     }
  };

void  Die  (const char * who)
  {
   fprintf (stderr, "ERROR:  %s: %s\n", who, gmg_last_error ());
   exit (EXIT_FAILURE);
  }

//  the extract options and the three paths of one job from  tok [0 .. n)
bool  Parse_Job  (const std::vector <std::string> & tok, Job_t & job, std::string & why)
  {
   std::vector <std::string>  pos;
   for  (size_t i = 0;  i < tok . size ();  i ++)
     {
      const std::string  & t = tok [i];
      if  (t == "-d" || t == "--dir")
          job . flags |= GMG_COORD_USE_DIR;
      else if  (t == "-s" || t == "--nostart")
          job . flags |= GMG_COORD_SKIP_START;
      else if  (t == "-t" || t == "--nostop")
          job . flags |= GMG_COORD_SKIP_STOP;
      else if  (t == "-w" || t == "--nowrap")
          job . flags |= GMG_COORD_NOWRAP;
      else if  (t == "--multi")
          job . multi = true;
      else if  (t == "-l" || t == "--minlen")
          {
           if  (i + 1 >= tok . size ())
               { why = "-l needs a number";  return  false; }
           job . min_len = strtol (tok [++ i] . c_str (), NULL, 10);
          }
      else if  (t . size () > 1 && t [0] == '-')
          { why = "unknown extract option " + t;  return  false; }
        else
          pos . push_back (t);
     }
   if  (pos . size () != 3)
       { why = "expected <sequence-file> <coords> <output.icm>";  return  false; }
   if  (job . multi)
       job . flags |= GMG_COORD_MULTI;
   job . seq_path = pos [0];
   job . coord_path = pos [1];
   job . out_path = pos [2];
   return  true;
  }

bool  Slurp  (const std::string & path, std::string & bytes)
  {
   FILE  * fp = fopen (path . c_str (), "rb");
   if  (fp == NULL)
       return  false;
   char  buf [1 << 16];
   size_t  n;
   bytes . clear ();
   while  ((n = fread (buf, 1, sizeof buf, fp)) > 0)
     bytes . append (buf, n);
   fclose (fp);
   return  true;
  }

void  Run_Job  (const Job_t & job, bool timing)
  {
   Laps_t  laps;

   std::string  bytes;
   if  (! Slurp (job . seq_path, bytes))
       {
        fprintf (stderr, "ERROR:  Could not open file  %s \n", job . seq_path . c_str ());
        exit (EXIT_FAILURE);
       }
   gmg_reads  * reads = NULL, * strings = NULL;
   gmg_fasta  * index = NULL;
   if  (gmg_fasta_ingest (bytes . data (), bytes . size (), & reads, & index) != GMG_OK)
       Die ("gmg_fasta_ingest");
   uint64_t  n_reads = 0, total = 0;
   gmg_fasta_info (index, & n_reads, & total, NULL);
   if  (n_reads == 0)
       {
        fprintf (stderr, "ERROR:  Failed to read file %s\n", job . seq_path . c_str ());
        exit (EXIT_FAILURE);
       }
   std::vector <uint64_t>  off (n_reads + 1);
   {
    std::vector <uint32_t>  words (gmg_packed_words (total));
    if  (gmg_reads_download (reads, words . data (), off . data ()) != GMG_OK)
        Die ("gmg_reads_download");
   }
   laps . Lap (0);

   //  the letters whose reverse-strand code is not the code complement
   uint64_t  n_amb = 0;
   gmg_fasta_ambiguous (bytes . data (), bytes . size (), NULL, NULL, 0, & n_amb);
   std::vector <uint64_t>  amb_base (n_amb ? n_amb : 1);
   std::vector <uint8_t>  amb_code (n_amb ? n_amb : 1);
   gmg_fasta_ambiguous (bytes . data (), bytes . size (), amb_base . data (), amb_code . data (), n_amb, & n_amb);

   //  --multi: the records by the first token of their header lines
   std::map <std::string, std::vector <uint32_t> >  by_tag;
   if  (job . multi)
       {
        std::vector <uint64_t>  hb (n_reads), he (n_reads);
        if  (gmg_fasta_headers (index, hb . data (), he . data ()) != GMG_OK)
            Die ("gmg_fasta_headers");
        for  (uint64_t r = 0;  r < n_reads;  r ++)
          {
           const std::string  hdr (bytes, hb [r], he [r] - hb [r]);
           const size_t  b = hdr . find_first_not_of (" \t\n");
           if  (b == std::string::npos)
               continue;
           const size_t  e = hdr . find_first_of (" \t\n", b);
           by_tag [hdr . substr (b, e == std::string::npos ? e : e - b)] . push_back (uint32_t (r));
          }
       }

   //  the coordinate lines, with the reference's formats and messages (src/Util/extract.cc:84-100, multi-extract.cc:76-93)
   FILE  * fp = (job . coord_path == "-" ? stdin : File_Open (job . coord_path . c_str (), "r"));
   std::vector <gmg_coord>  coords;
   std::vector <std::string>  coord_text;
   char  line [MAX_LINE], tag [MAX_LINE], id [MAX_LINE];
   const bool  use_dir = (job . flags & GMG_COORD_USE_DIR) != 0;
   while  (fgets (line, MAX_LINE, fp) != NULL)
     {
      long int  start, end;
      int  dir = 0, got, want;
      if  (job . multi)
          {
           want = (use_dir ? 5 : 4);
           got = (use_dir ? sscanf (line, "%s %s %ld %ld %d", id, tag, & start, & end, & dir)
                          : sscanf (line, "%s %s %ld %ld", id, tag, & start, & end));
          }
        else
          {
           want = (use_dir ? 4 : 3);
           got = (use_dir ? sscanf (line, "%s %ld %ld %d", tag, & start, & end, & dir)
                          : sscanf (line, "%s %ld %ld", tag, & start, & end));
          }
      if  (got != want)
          {
           fprintf (stderr, "ERROR:  Skipped following coord line\n");
           fputs (line, stderr);
           continue;
          }
      gmg_coord  c;
      c . dir = dir;
      c . start = start;
      c . end = end;
      if  (! job . multi)
          {
           c . read = 0;
           coords . push_back (c);
           coord_text . push_back (line);
           continue;
          }
      std::map <std::string, std::vector <uint32_t> > :: const_iterator  it = by_tag . find (tag);
      if  (it == by_tag . end ())
          continue;
      for  (size_t k = 0;  k < it -> second . size ();  k ++)
        {
         c . read = it -> second [k];
         coords . push_back (c);
         coord_text . push_back (line);
        }
     }
   if  (fp != stdin)
       fclose (fp);

   std::vector <gmg_gene_region>  regions (coords . size () ? coords . size () : 1);
   std::vector <uint64_t>  line_of (coords . size () ? coords . size () : 1);
   uint64_t  n_regions = 0;
   if  (gmg_extract_plan (off . data (), n_reads, coords . data (), coords . size (), job . flags, job . min_len,
                          regions . data (), line_of . data (), & n_regions) != GMG_OK)
       {
        //  the message names the entry of  coords ; show the line it came from
        const char  * msg = gmg_last_error ();
        const char  * p = strstr (msg, "line ");
        const unsigned long long  k = (p != NULL ? strtoull (p + 5, NULL, 10) : 0);
        fprintf (stderr, "ERROR:  %s\n", msg);
        if  (k < coord_text . size ())
            fprintf (stderr, "coordinate line:  %s", coord_text [k] . c_str ());
        exit (EXIT_FAILURE);
       }
   laps . Lap (1);

   if  (n_regions == 0)
       {
        fprintf (stderr, "ERROR:  Cannot create model--no input data\n");
        exit (EXIT_FAILURE);
       }
   if  (gmg_reads_extract (reads, regions . data (), n_regions, Reverse_Strings ? GMG_EXTRACT_REVERSED : 0,
                           n_amb ? amb_base . data () : NULL, n_amb ? amb_code . data () : NULL, n_amb, & strings) != GMG_OK)
       Die ("gmg_reads_extract");
   laps . Lap (2);

   ICM_Training_t  model (Model_Len, Model_Depth, Model_Periodicity);
   std::string  err;
   if  (! model . Try_Train_Reads (strings, err))
       {
        fprintf (stderr, "ERROR:  %s\n", err . c_str ());
        exit (EXIT_FAILURE);
       }
   laps . Lap (3);

   FILE  * output_fp;
   if  (job . out_path == "-")
       output_fp = stdout;
     else
       output_fp = File_Open (job . out_path . c_str (), Print_Binary ? "wb" : "w");
   model . Output (output_fp, Print_Binary);
   if  (output_fp != stdout)
       fclose (output_fp);
     else
       fflush (stdout);
   gmg_reads_free (strings);
   gmg_reads_free (reads);
   gmg_fasta_free (index);
   laps . Lap (4);
   if  (timing)
       fprintf (stderr, "[build-icm_gpu] %s: %llu regions  ingest %.3f ms  plan %.3f ms  extract %.3f ms  train %.3f ms  write %.3f ms\n",
                job . out_path . c_str (), (unsigned long long) n_regions, laps . ms [0], laps . ms [1], laps . ms [2], laps . ms [3], laps . ms [4]);
  }

}  // namespace


int  main
    (int argc, char * argv [])
  {
   //  our own options come off before the reference's parser sees the rest
   int  split = -1;
   bool  list = false, timing = false;
   std::vector <char *>  args;
   for  (int i = 0;  i < argc;  i ++)
     {
      if  (i > 0 && split < 0 && strcmp (argv [i], "--timing") == 0)
          { timing = true;  continue; }
      if  (i > 0 && split < 0 && (strcmp (argv [i], "--extract") == 0 || strcmp (argv [i], "--list") == 0))
          {
           split = i;
           list = (strcmp (argv [i], "--list") == 0);
           break;
          }
      args . push_back (argv [i]);
     }
   if  (split < 0)
       {
        args . push_back (NULL);
        return  build_icm_reference_main (int (args . size ()) - 1, & args [0]);      // stdin to model
       }

   std::vector <Job_t>  jobs;
   std::string  why;
   if  (! list)
       {
        std::vector <std::string>  tok;
        for  (int i = split + 1;  i < argc;  i ++)
          if  (strcmp (argv [i], "--timing") == 0)
              timing = true;
            else
              tok . push_back (argv [i]);
        Job_t  job;
        if  (! Parse_Job (tok, job, why))
            {
             fprintf (stderr, "ERROR:  --extract: %s\n", why . c_str ());
             Usage (argv [0]);
             exit (EXIT_FAILURE);
            }
        jobs . push_back (job);
       }
     else
       {
        if  (split + 2 != argc)
            {
             fprintf (stderr, "ERROR:  --list takes one file of jobs\n");
             exit (EXIT_FAILURE);
            }
        FILE  * fp = File_Open (argv [split + 1], "r");
        char  line [MAX_LINE];
        int  line_no = 0;
        while  (fgets (line, MAX_LINE, fp) != NULL)
          {
           line_no ++;
           std::vector <std::string>  tok;
           for  (char * p = strtok (line, " \t\r\n");  p != NULL;  p = strtok (NULL, " \t\r\n"))
             tok . push_back (p);
           if  (tok . empty () || tok [0] [0] == '#')
               continue;
           Job_t  job;
           if  (! Parse_Job (tok, job, why))
               {
                fprintf (stderr, "ERROR:  %s line %d: %s\n", argv [split + 1], line_no, why . c_str ());
                exit (EXIT_FAILURE);
               }
           jobs . push_back (job);
          }
        fclose (fp);
       }

   //  the reference's parser wants its one positional argument: the output file of the (first) job
   static char  placeholder [] = "-";
   args . push_back (jobs . empty () ? placeholder : strdup (jobs [0] . out_path . c_str ()));
   args . push_back (NULL);
   Parse_Command_Line (int (args . size ()) - 1, & args [0]);
   if  (Skip_In_Frame_Stop_Strings)
       {
        fprintf (stderr, "ERROR:  -F needs the letters of the training strings; it cannot be combined with --extract / --list\n"
                         "        (use  extract ... | build-icm -F ...)\n");
        exit (2);
       }

   const char  * dev = getenv ("GMG_DEVICE");
   if  (gmg_init (dev ? atoi (dev) : 0) != GMG_OK)
       Die ("gmg_init");
   for  (size_t j = 0;  j < jobs . size ();  j ++)
     Run_Job (jobs [j], timing);

   return  0;
  }
