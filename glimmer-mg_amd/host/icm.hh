//  icm.hh -- MI355X-native drop-in for the reference's Interpolated Context
//  Model classes (scoring: ICM_t; training: ICM_Training_t).
//
//  Same public interface, constants, field names and error behaviour as the
//  reference's  ICM_t  (src/ICM/icm.hh:26-84,106-180,303), so that code written
//  against it (src/Glimmer/glimmer3.cc, glimmer-mg.cc, glimmer_base.cc,
//  src/ICM/build-icm.cc) recompiles unchanged -- and so do src/ICM/build-fixed.cc and
//  src/ICM/score-fixed.cc, through the fixed-length classes below (Fixed_Length_ICM_t,
//  Fixed_Length_ICM_Training_t, src/ICM/icm.hh:216-289).  Everything that computes a
//  score goes through the extern "C" HIP layer declared in include/gmg.h;
//  there is no CPU scoring path in this class.  Model I/O and the null-model
//  builder are host code, as in the reference.
//
//  Additions (not in the reference) are grouped at the end of the class:
//  batch entry points and access to the device mirror.

#ifndef GMG_HOST_ICM_HH_INCLUDED
#define GMG_HOST_ICM_HH_INCLUDED

#include <stdio.h>
#include <string>
#include <vector>

struct gmg_model;   // include/gmg.h
struct gmg_reads;
struct gmg_fixed_model;

// ---- constants of src/ICM/icm.hh:21-80 (callers and the training code use them) ----
#define  STORE_MUT_INFO  1
const int  ALPHABET_SIZE = 4;
const int  ALPHA_SQUARED = (ALPHABET_SIZE * ALPHABET_SIZE);
const char  ALPHA_STRING [] = "acgt";
const int  DEFAULT_MODEL_LEN = 12;
const int  ID_STRING_LEN = 150;
const int  DEFAULT_MODEL_DEPTH = 7;
const unsigned  NUM_FIXED_LENGTH_PARAMS = 6;
const int  DEFAULT_PERIODICITY = 3;
const char  MAX_MI_CHAR = '*';
const char  SEPARATOR_CHAR = '|';
const int  ICM_VERSION_ID = 200;
//  used by the training side and by glimmer3's Integerize_Scores (glimmer3.cc:627)
const int  NUM_CHI2_ENTRIES = 7;
const float  CHI2_VAL [NUM_CHI2_ENTRIES] = {2.37, 4.11, 6.25, 7.81, 9.35, 11.3, 12.8};
const float  CHI2_SIGNIFICANCE [NUM_CHI2_ENTRIES] = {0.50, 0.75, 0.90, 0.95, 0.975, 0.99, 0.995};
const double  MUT_INFO_BIAS = 0.03;
const double  MAX_LOG_DIFF = -46.0;
const double  MUT_INFO_EPSILON = 1e-4;
const double  PSEUDO_COUNT = 0.001;
const int  SAMPLE_SIZE_BOUND = 400;

#define  PARENT(x) ((int) ((x) - 1) / ALPHABET_SIZE)

//  src/ICM/icm.hh:91-92
enum  ICM_Model_t
    {UNKNOWN_TYPE};


//  src/ICM/icm.hh:106-113 (STORE_MUT_INFO = 1 layout, 24 bytes)
struct  ICM_Score_Node_t
  {
   short int  mut_info_pos;
   float  mut_info;
   float  prob [ALPHABET_SIZE];
  };


class  ICM_t
  {
  protected:
   bool  empty;
   int  model_len;
   int  model_depth;
   int  periodicity;
   int  num_nodes;
   ICM_Score_Node_t  * * score;

  public:
   ICM_t
       (int m = DEFAULT_MODEL_LEN,
        int d = DEFAULT_MODEL_DEPTH,
        int p = DEFAULT_PERIODICITY);
   ~ ICM_t
       ();

   int  Get_Model_Len
       (void)
     { return  model_len; }
   int  Get_Periodicity
       (void)
     { return  periodicity; }

   void  Build_Indep_WO_Stops
       (double gc_frac, const std::vector <const char *> & stop_codon);
   void  Build_Reverse_Codon_WO_Stops
       (double codon_prob [64], const std::vector <const char *> & stop_codon);
   void  Cumulative_Score
       (const std::string & s, std::vector <double> & score, int frame)  const;
   void  Cumulative_Score_String
       (char * string, int len, int frame, double * score);
   void  Display
       (FILE * fp);
   void  Frame_Score
       (const std::string & s, std::vector <double> & score, int frame)  const;
   void  Full_Window_Distrib
       (char * string, int frame, float * dist);
   double  Full_Window_Prob
       (const char * string, int frame)  const;
   void  Input
       (FILE * fp);
   void  Output
       (FILE * fp, bool binary_form);
   void  Output_Node
       (FILE * fp, ICM_Score_Node_t * node, int id, int frame, bool binary_form);
   double  Partial_Window_Prob
       (int predict_pos, const char * string, int frame)  const;
   void  Read
       (char * path);
   double  Score_String
       (const char * string, int len, int frame)  const;
   void  Set_Label_String
       (char * label, int id, int frame);
   void  Write_Header
       (FILE * fp, bool binary_form);
   void Copy
       (ICM_t & icm);

   // ---- additions ---------------------------------------------------------
   //  Parse an .icm stream without exiting: returns false and sets  err .
   bool  Try_Input
       (FILE * fp, std::string & err);
   //  Flat copies of the tables in the layout gmg_model_upload() takes.
   void  Export_Tables
       (std::vector <short> & mip, std::vector <float> & prob4)  const;
   int  Get_Model_Depth  (void)  const  { return  model_depth; }
   int  Get_Num_Nodes  (void)  const  { return  num_nodes; }
   bool  Is_Empty  (void)  const  { return  empty; }
   //  Device mirror of the tables (uploaded on first use, dropped whenever the
   //  tables change through this class).  Code that edits  score  directly
   //  (a training subclass) must call Invalidate_Device_Mirror() afterwards.
   const gmg_model *  Device_Model  (void)  const;
   void  Invalidate_Device_Mirror  (void)  const;

  private:
   mutable gmg_model  * dev_mirror;
   void  Free_Tables  (void);
   void  Alloc_Tables  (void);
   void  Build_From_Codon_Probs
       (double codon_prob [64], const std::vector <const char *> & stop_codon, const char * who);
  };


//  src/ICM/icm.hh:183-213.  Same constructor and Train_Model as the reference's training class, so that
//  src/ICM/build-icm.cc recompiles against this header unchanged.  The pair counting of every tree level
//  (Count_Char_Pairs, Count_Char_Pairs_Restricted, Get_Training_Node; src/ICM/icm.cc:1190-1256,1841-1870) runs on
//  the device through gmg_trainer_* (include/gmg.h) -- there is no CPU counting path; choosing each node's context
//  position and the chi-squared interpolation (src/ICM/icm.cc:1061-1186,1260-1352) are per-node host arithmetic as
//  in the reference (icm_train.cc).  The reference's per-node count tables (ICM_Training_Node_t, 46 MB for the
//  default shape) are not kept: a level's counts live in HBM while that level is built.
class  ICM_Training_t  :  public ICM_t
  {
  public:
   ICM_Training_t
       (int m = DEFAULT_MODEL_LEN,
        int d = DEFAULT_MODEL_DEPTH,
        int p = DEFAULT_PERIODICITY);
   ~ ICM_Training_t
       ();

   void  Train_Model
       (const std::vector <char *> & data);

   // ---- additions ---------------------------------------------------------
   //  Train_Model without the exit: returns false and sets  err  when the device layer fails.
   bool  Try_Train_Model
       (const char * const * data, int string_ct, std::string & err);
   //  the same from training strings that are already a batch on the device (gmg_reads_extract, gmg_reads_upload ...):
   //  everything of Try_Train_Model behind its upload.   strings  stays the caller's.
   bool  Try_Train_Reads
       (const gmg_reads * strings, std::string & err);
  };


//  src/ICM/icm.hh:216-255.  A fixed-length model of  length  L: sub-model i (0-based) is an ICM_t of model_len i+1,
//  periodicity 1, that predicts base i of the window after Permute_String.  Score_Window / subrange_score are ONE
//  gmg_fixed_score call each (include/gmg.h: the window, its permutation and all L descents on the device); the batch form
//  Score_Windows is one call for all its strings.  Deviations from the reference: L must be 1..32 (a window of 2-bit codes
//  fits one 64-bit register) and the permutation must be a bijection of 0..L-1 -- both are refused with a message and
//  exit(EXIT_FAILURE) where the reference reads on (and has undefined behaviour); every sub-model must have the shape the
//  training class writes (model_len i+1, periodicity 1).  Subscript maps every character to a base
//  (tolower (Filter (ch)), '\0' included), so the only character error of Score_Window / subrange_score is the
//  reference's "too short" check on the permuted window.
class  Fixed_Length_ICM_t
  {
  private:
   int  length;
   int  max_depth;
   int  special_position;
   ICM_Model_t  model_type;
   int  * permutation;
   std::vector <ICM_t *> sub_model;

  public:
   Fixed_Length_ICM_t
       (int len = 1, int sp = 0, int * perm = NULL, ICM_Model_t = UNKNOWN_TYPE);
   ~ Fixed_Length_ICM_t
       ();

   int  Get_Length
       (void)
     { return  length; }
   double  Score_Window
       (char * w);

   // Match MDD_t interface
   int  getModelLength
       (void)
     { return  length; }
   int  getModelType
       (void)
     { return  model_type; }
   int  getSpecialPosition
       (void)
     { return  special_position; }
   void  read
       (const char * path);
   double  subrange_score
       (char * w, int lo, int hi);
   double  score
       (char * w)
     { return  Score_Window (w); }

   // ---- additions ---------------------------------------------------------
   //  read without the exit: returns false and sets  err  (the message the reference would print)
   bool  Try_Read
       (const char * path, std::string & err);
   //  the same on an open stream (the bytes of one model are consumed)
   bool  Try_Input
       (FILE * fp, std::string & err);
   //  out [k] = subrange_score (strings [k], lo, hi) for k < n, in ONE device call.  Exits as subrange_score would at the first
   //  string it would stop at; Try_Score_Windows returns false and sets  err  instead.
   void  Score_Windows
       (const char * const * strings, int n, int lo, int hi, double * out);
   bool  Try_Score_Windows
       (const char * const * strings, int n, int lo, int hi, double * out, std::string & err);
   int  Get_Max_Depth  (void)  const  { return  max_depth; }
   //  the permutation as read (identity when the model has none); NULL before read
   const int *  Get_Permutation  (void)  const  { return  permutation; }
   const ICM_t *  Get_Sub_Model  (int i)  const  { return  sub_model [i]; }
   //  Device copy of all L sub-models and the permutation (uploaded on first use, dropped by read)
   const gmg_fixed_model *  Device_Model  (void)  const;
   //  the reference's "too short" check of subrange_score (w, lo, hi) alone: false and its message when it would stop there
   bool  Check_Window  (const char * w, int lo, int hi, std::string & err)  const;

  private:
   mutable gmg_fixed_model  * dev_fixed;
   void  Clear  (void);
  };


//  src/ICM/icm.hh:258-289.  Train_Model permutes the caller's strings in place, as the reference does, then trains
//  sub-model i (1 <= i <= length) as ICM_Training_t (i, min (i - 1, max_depth), 1) on the length-i prefixes: the device
//  counting of ICM_Training_t, L times.  Output / Write_Header write the reference's bytes (binary, and -t text).
class  Fixed_Length_ICM_Training_t
  {
  private:
   int  length;
   int  max_depth;
   int  special_position;
   ICM_Model_t  model_type;
   int  * permutation;
   std::vector <ICM_Training_t *> sub_model;

  public:
   Fixed_Length_ICM_Training_t
       (int len, int md, int sp, int * perm, ICM_Model_t mt = UNKNOWN_TYPE);
   ~ Fixed_Length_ICM_Training_t
       ();
   void  Output
       (FILE * fp, bool binary_form);
   void  Train_Model
       (std::vector <char *> & data);
   void  Write_Header
       (FILE * fp, bool binary_form);

   // ---- additions ---------------------------------------------------------
   //  Train_Model without the exit: returns false and sets  err  when the device layer fails
   bool  Try_Train_Model
       (std::vector <char *> & data, std::string & err);
  };


void  Permute_Data
    (std::vector <char *> & data, int * perm);
void  Permute_String
    (char * s, int * perm, int n);


int  Subscript
    (char ch);

#endif
