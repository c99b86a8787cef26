//  long-orfs_gpu.cc -- the reference's long-orfs (src/Glimmer/long-orfs.cc) with its entropy distance ratios taken from the device:
//  the amino-acid counts of every ORF of orf_list come from ONE gmg_entropy_regions call, the reference's arithmetic finishes them
//  on the host (gmg_entropy_from_counts: the same libm, the same order of operations), and Entropy_Filter's keep / drop decision
//  and the printed %6.3f column use those values -- the output is byte-identical by construction.  The regions that are printed
//  are regions of the ORF list, so their values are looked up; only a run without -t, which scores nothing before its output,
//  asks the device a second time.  Parse_Command_Line, Find_Orfs, Get_Intervals, Find_Optimal_Len, Remove_Shorter,
//  Eliminate_Overlapping and the Echo_* functions are the reference's own and run on the host (one linear pass over a genome is
//  milliseconds there): the file is pulled in whole with its main renamed (integration/Makefile).
//
//      long-orfs_gpu [--multi] <long-orfs options> <sequence-file> <output-file>          (GMG_DEVICE selects the GPU)
//
//  The reference reads the FIRST record of its input.  With --multi every record of a multi-fasta file is treated as the reference
//  treats a file that holds this record alone (Min_Gene_Len starts again from its -g value), the ORFs of all records go to the
//  device in one call, and the output is, per record, a line ">" + its header followed by what the reference writes for it (with
//  headers: the general settings once, in front).  A record on which the reference would stop -- shorter than the minimum gene
//  length, or no ORF below the entropy cutoff -- keeps its header line and no rows.
//
//  For ONE bacterial genome the reference needs 0.16 s, which is about what starting the HIP runtime costs: the single-genome
//  form exists for parity, the throughput cases are --multi on an assembly and the batch entry points.

#include "../include/gmg.h"

#include <map>
#include <string>
#include <utility>
#include <vector>

#define main long_orfs_reference_main
#include "long-orfs.cc"
#undef main

namespace {

struct Record_t
  {
   string  seq, hdr;
   vector <Orf_t>  orf_list;
   vector <Orf_Interval_t>  interval;
   int  final_min_len;
   bool  stopped;        // the reference would have thrown on this record
   size_t  read;         // its read in the device batch
  };

typedef std::pair <int, std::pair <int, int> >  Region_Key_t;      // (first, (len, strand))

void  Die  (const char * who)
  {
   fprintf (stderr, "ERROR:  %s: %s\n", who, gmg_last_error ());
   exit (EXIT_FAILURE);
  }

//  The region Entropy_Distance_Ratio (start, len, fr) reads: 0-based first base, length, strand
gmg_gene_region  Make_Region  (size_t read, int start, int len, int fr)
  {
   gmg_gene_region  r;
   r . read = uint32_t (read);
   r . first = On_Seq_0 (start - 1);
   r . len = len;
   r . strand = fr > 0 ? 1 : -1;
   return  r;
  }

//  Entropy_Filter's region of an ORF (long-orfs.cc:370-377)
gmg_gene_region  Orf_Region  (size_t read, const Orf_t & orf)
  {
   const int  stop = orf . Get_Stop_Position (), len = orf . Get_Gene_Len (), frame = orf . Get_Frame ();
   return  Make_Region (read, frame > 0 ? On_Seq_1 (stop - len) : On_Seq_1 (stop + len + 2), len, frame);
  }

//  Output_Orfs' coordinates of an interval (long-orfs.cc:1089-1117)
void  Interval_Coords  (const Orf_Interval_t & iv, int & start, int & stop, int & len)
  {
   len = iv . hi - iv . lo;
   if  (iv . frame > 0)
       {
        stop = Without_Stops ? On_Seq_1 (iv . hi) : On_Seq_1 (iv . hi + 3);
        start = Without_Stops ? On_Seq_1 (stop - len + 1) : On_Seq_1 (stop - len - 2);
       }
     else
       {
        stop = Without_Stops ? On_Seq_1 (iv . lo + 1) : On_Seq_1 (iv . lo - 2);
        start = Without_Stops ? On_Seq_1 (stop + len - 1) : On_Seq_1 (stop + len + 2);
       }
  }

//  The device side: the records as one batch of reads, made at the first call
struct Device_t
  {
   gmg_reads  * reads;
   char  aa [64];
   Device_t  ()  : reads (NULL)  {}

   void  Open  (const vector <Record_t> & rec)
     {
      const char  * dev = getenv ("GMG_DEVICE");
      if  (gmg_init (dev ? atoi (dev) : 0) != GMG_OK)
          Die ("gmg_init");
      if  (gmg_xlate_table (Genbank_Xlate_Code, aa) != GMG_OK)
          {
           sprintf (Clean_Exit_Msg_Line, "ERROR:  Bad translation table = %d", Genbank_Xlate_Code);
           SIMPLE_THROW (Clean_Exit_Msg_Line);
          }
      const size_t  n = rec . size ();
      vector <uint64_t>  off (n + 1, 0);
      for  (size_t k = 0;  k < n;  k ++)
        off [k + 1] = off [k] + rec [k] . seq . length ();
      vector <uint32_t>  packed (gmg_packed_words (off [n]), 0);
      for  (size_t k = 0;  k < n;  k ++)
        gmg_pack_bases (rec [k] . seq . data (), rec [k] . seq . length (), off [k], & packed [0]);
      if  (gmg_reads_upload (& packed [0], & off [0], n, & reads) != GMG_OK)
          Die ("gmg_reads_upload");
     }

   //  ratio [k] of regions [k]: counts from the device, the reference's arithmetic on the host
   void  Ratios  (const vector <Record_t> & rec, const vector <gmg_gene_region> & regions, vector <double> & ratio)
     {
      const size_t  n = regions . size ();
      ratio . resize (n);
      if  (n == 0)
          return;
      if  (reads == NULL)
          Open (rec);
      int32_t  * d_counts;
      vector <int32_t>  counts (n * 20);
      if  (gmg_device_malloc ((void * *) & d_counts, n * 20 * sizeof (int32_t)) != GMG_OK)
          Die ("gmg_device_malloc");
      if  (gmg_entropy_regions (reads, & regions [0], n, aa, Pos_Entropy_Profile, Neg_Entropy_Profile, d_counts, NULL, NULL) != GMG_OK)
          Die ("gmg_entropy_regions");
      if  (gmg_memcpy_d2h (& counts [0], d_counts, n * 20 * sizeof (int32_t), NULL) != GMG_OK)
          Die ("gmg_memcpy_d2h");
      gmg_device_free (d_counts);
      for  (size_t k = 0;  k < n;  k ++)
        gmg_entropy_from_counts (& counts [20 * k], Pos_Entropy_Profile, Neg_Entropy_Profile, NULL, NULL, & ratio [k]);
     }

   void  Close  ()
     {
      if  (reads != NULL)
          gmg_reads_free (reads);
      reads = NULL;
     }
  };

//  the globals of the reference that belong to one record
void  Select_Record  (const Record_t & r, int min_gene_len)
  {
   Sequence = r . seq;
   Sequence_Len = Sequence . length ();
   Fasta_Header = r . hdr . c_str ();
   Min_Gene_Len = min_gene_len;
  }

}  // namespace

int  main
    (int argc, char * argv [])
  {
   try
     {
      FILE  * sequence_fp, * output_fp;
      vector <Record_t>  rec;
      vector <char *>  args;
      bool  multi = false;
      string  seq, hdr;
      time_t  now;

      now = time (NULL);
      cerr << "Starting at " << ctime (& now) << endl;

      Verbose = 0;

      for  (int i = 0;  i < argc;  i ++)
        if  (i > 0 && strcmp (argv [i], "--multi") == 0)
            multi = true;
          else
            args . push_back (argv [i]);
      args . push_back (NULL);
      Parse_Command_Line (int (args . size ()) - 1, & args [0]);
      const int  initial_min_gene_len = Min_Gene_Len;

      if  (Ignore_File_Name != NULL)
          Get_Ignore_Regions ();

      Set_Start_And_Stop_Codons ();

      if  (strcmp (Output_Filename, "-") == 0)
          output_fp = stdout;
        else
          output_fp = File_Open (Output_Filename, "w", __FILE__, __LINE__);

      Echo_General_Settings (stderr);
      if  (Print_Output_Header)
          Echo_General_Settings (output_fp);

      sequence_fp = File_Open (Sequence_File_Name, "r", __FILE__, __LINE__);

      while  (Fasta_Read (sequence_fp, seq, hdr))
        {
         Record_t  r;
         r . seq = seq;
         for  (size_t i = 0;  i < r . seq . length ();  i ++)
           r . seq [i] = Filter (tolower (r . seq [i]));
         r . hdr = hdr;
         r . final_min_len = initial_min_gene_len;
         r . stopped = false;
         r . read = rec . size ();
         rec . push_back (r);
         if  (! multi)
             break;
        }
      fclose (sequence_fp);
      if  (rec . size () == 0)
          SIMPLE_THROW ("ERROR:  Failed to read input sequence");

      //  the ORFs of every record on the host, their regions as one list
      Device_t  device;
      vector <gmg_gene_region>  regions;
      vector <double>  ratio;
      for  (size_t k = 0;  k < rec . size ();  k ++)
        {
         Select_Record (rec [k], initial_min_gene_len);
         Find_Orfs (rec [k] . orf_list);
         if  (Use_Entropy_Filter)
             for  (size_t i = 0;  i < rec [k] . orf_list . size ();  i ++)
               regions . push_back (Orf_Region (k, rec [k] . orf_list [i]));
        }
      device . Ratios (rec, regions, ratio);

      //  Entropy_Filter (long-orfs.cc:355-389) with those values, then the reference's interval steps, record by record
      vector <std::map <Region_Key_t, double> >  known (rec . size ());
      vector <gmg_gene_region>  wanted;
      size_t  next = 0;
      for  (size_t k = 0;  k < rec . size ();  k ++)
        {
         Record_t  & r = rec [k];
         Select_Record (r, initial_min_gene_len);
         if  (Use_Entropy_Filter)
             {
              size_t  j = 0;
              for  (size_t i = 0;  i < r . orf_list . size ();  i ++, next ++)
                {
                 const gmg_gene_region  & g = regions [next];
                 known [k] [Region_Key_t (g . first, std::make_pair (g . len, g . strand))] = ratio [next];
                 if  (ratio [next] < Entropy_Cutoff)
                     {
                      if  (i != j)
                          r . orf_list [j] = r . orf_list [i];
                      j ++;
                     }
                }
              r . orf_list . resize (j);
             }
         if  (r . orf_list . size () == 0)
             {
              if  (! multi)
                  SIMPLE_THROW ("ERROR:  No valid orfs found below entropy cutoff");
              r . stopped = true;
              continue;
             }

         Get_Intervals (r . interval, r . orf_list);
         if  (! Fixed_Min_Len)
             {
              const int  optimal_len = Find_Optimal_Len (r . interval);
              Remove_Shorter (r . interval, optimal_len);
              Min_Gene_Len = optimal_len;
             }
         r . final_min_len = Min_Gene_Len;
         Eliminate_Overlapping (r . interval, Max_Olap_Bases);

         for  (size_t i = 0;  i < r . interval . size ();  i ++)
           {
            int  start, stop, len;
            Interval_Coords (r . interval [i], start, stop, len);
            const gmg_gene_region  g = Make_Region (k, start, len, r . interval [i] . frame);
            if  (known [k] . count (Region_Key_t (g . first, std::make_pair (g . len, g . strand))) == 0)
                wanted . push_back (g);
           }
        }
      device . Ratios (rec, wanted, ratio);
      for  (size_t i = 0;  i < wanted . size ();  i ++)
        known [wanted [i] . read] [Region_Key_t (wanted [i] . first, std::make_pair (wanted [i] . len, wanted [i] . strand))] = ratio [i];
      device . Close ();

      //  the output, as Echo_Specific_Settings and Output_Orfs write it
      for  (size_t k = 0;  k < rec . size ();  k ++)
        {
         Record_t  & r = rec [k];
         Select_Record (r, r . final_min_len);
         if  (multi)
             fprintf (output_fp, ">%s\n", r . hdr . c_str ());
         if  (r . stopped)
             continue;

         Echo_Specific_Settings (stderr, Sequence_Len);
         if  (Print_Output_Header)
             {
              Echo_Specific_Settings (output_fp, Sequence_Len);
              fprintf (output_fp, "\nPutative Genes:\n");
             }
         int  total_len = 0;
         for  (size_t i = 0;  i < r . interval . size ();  i ++)
           {
            int  start, stop, len;
            Interval_Coords (r . interval [i], start, stop, len);
            total_len += len;
            const gmg_gene_region  g = Make_Region (k, start, len, r . interval [i] . frame);
            fprintf (output_fp, "%05d %7d %7d  %+2d  %6.3f\n", int (i) + 1, start, stop, r . interval [i] . frame,
                     known [k] [Region_Key_t (g . first, std::make_pair (g . len, g . strand))]);
           }
         fprintf (stderr, "Number of genes = %d\n", int (r . interval . size ()));
         fprintf (stderr, "Total bases = %d\n", total_len);
        }

      fclose (output_fp);
     }
   catch (std :: exception & e)
     {
      cerr << "** Standard Exception **" << endl;
      cerr << e << endl;
      exit (EXIT_FAILURE);
     }

   return  0;
  }
