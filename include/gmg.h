/*
 * gmg.h -- C ABI of the MI355X (gfx950) IMM scorer for Glimmer-MG.
 *
 * This is the drop-in boundary: a thin extern "C" layer over hand-written HIP
 * kernels.  Plain pointers and sizes only; no C++ or torch types.  The host
 * side (glimmer-mg_amd/host/icm.hh, an ICM_t with the reference's public
 * interface) and any FFI binding call exactly these entry points.
 *
 * Each entry point cites the reference interface it replaces
 * (paths relative to the reference root, davek44/Glimmer-MG).
 *
 * Conventions
 *   - every function returns 0 (GMG_OK) or a negative gmg_status; it never
 *     calls exit().  gmg_last_error() gives the text for the calling thread.
 *   - "d_" pointers are device (HBM) pointers owned by the caller (hipMalloc /
 *     torch); all other pointers are host memory, caller-owned.
 *   - handles (gmg_model, gmg_reads, gmg_segments) own their device memory.
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream; gmg_stream_create
 *     hands out non-blocking ones, which are NOT ordered with the default stream).  Every
 *     kernel, copy and memset of a call that takes a stream runs on that stream or on side
 *     streams joined to it by events; nothing goes through the default stream.  Whether a
 *     call returns before its work is done is said per entry point (DESIGN.md 2.3 has the
 *     table): the scoring calls that write to d_ pointers do, the calls that return host
 *     results or result handles wait for the stream.
 *   - an entry point WITHOUT a stream parameter that makes a handle (the _upload, _create,
 *     _wrap_device, _select, _extract, _splice, _build, _from_tables calls) works on the
 *     default stream and has waited for it when it returns: the handle may be used on any
 *     stream at once.
 *   - host threads: any number of host threads may call any entry point at the same
 *     time, provided no two calls share a stream (the default stream included) or a mutable handle.
 *     Mutable handles belong to ONE call at a time: gmg_letters (its device text is valid until the
 *     next text call), gmg_tophits, gmg_trainer, gmg_single (one per host thread), gmg_orf_batch
 *     (between _begin and _fetch), gmg_model_set (until _finish).  Const handles may be shared freely:
 *     gmg_model, gmg_null_set, gmg_fixed_model, gmg_reads, gmg_segments, gmg_mg_result, gmg_fasta,
 *     gmg_audit, gmg_windows, gmg_gaps, gmg_features, gmg_classes -- and the host classes ICM_t and
 *     Fixed_Length_ICM_t through their const scoring methods, the first-use upload of their device
 *     mirror included.  gmg_set_option is process-wide: set options while no call is running.
 *     gmg_last_error() is the calling thread's own text.  A thread that ends gives back everything
 *     the library made for it (side streams, events, staging).
 *   - base code: a=0 c=1 g=2 t=3 (ALPHA_STRING, src/ICM/icm.hh:30), complement
 *     = 3 - code.  Packed reads hold 16 bases per uint32, base g of the job at
 *     bits [2*(g%16), 2*(g%16)+1] of word g/16, reads concatenated without
 *     padding; base_offsets[r] is the job-wide index of read r's first base
 *     (n_reads+1 entries).
 */
#ifndef GMG_H
#define GMG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum gmg_status {
    GMG_OK = 0,
    GMG_EINVAL = -1,     /* bad argument (NULL handle, frame out of range, ...)          */
    GMG_ENODEV = -2,     /* no usable gfx950 device / HIP runtime failure at init         */
    GMG_ENOMEM = -3,     /* host or device allocation failed                              */
    GMG_EHIP = -4,       /* a HIP call failed; text in gmg_last_error()                   */
    GMG_EBADMODEL = -5,  /* model parameters outside what the kernels support             */
    GMG_ERANGE = -6,     /* a segment / window reaches outside its read                   */
    GMG_ETOOBIG = -7     /* the batch would hold more ORFs or starts than the 32-bit index fields of the result
                            records address (gmg_mg_orf.start_begin, gmg_orf_result.start_begin): nothing wraps,
                            the call refuses -- score the reads in smaller batches (gmg_shard_plan)              */
} gmg_status;

typedef struct gmg_model gmg_model;       /* device copy of one ICM_t table set  */
typedef struct gmg_reads gmg_reads;       /* device copy of a batch of reads     */
typedef struct gmg_segments gmg_segments; /* device copy of a list of segments   */

/* A scoring buffer cut from a read, in the orientation the reference scores it
 * (src/Glimmer/glimmer3.cc:1322-1343, src/Glimmer/glimmer-mg.cc:1482,1497):
 *   GMG_REVERSED     B[j] = S[lo+len-1-j]        Reverse_Transfer     (glimmer_base.cc:2505-2533)
 *   GMG_COMPLEMENTED B[j] = comp(S[lo+j])        Complement_Transfer  (glimmer_base.cc:410-434)
 *   GMG_FORWARD      B[j] = S[lo+j]              the string as given  (Score_String on a read)
 *   GMG_REVCOMP      B[j] = comp(S[lo+len-1-j])  Reverse_Complement_Transfer (glimmer_base.cc:2484-2501)
 * Context never crosses the start of the buffer: the first model_len-1 bases of
 * every segment use the partial-window rule (src/ICM/icm.cc:807-842). */
typedef enum gmg_orient {
    GMG_FORWARD = 0,
    GMG_REVERSED = 1,
    GMG_COMPLEMENTED = 2,
    GMG_REVCOMP = 3
} gmg_orient;

typedef struct gmg_segment {
    uint32_t read;    /* index into the gmg_reads batch            */
    uint32_t lo;      /* first base of the region, 0-based in read */
    uint32_t len;     /* number of bases                           */
    uint32_t orient;  /* gmg_orient                                */
} gmg_segment;

/* ---- library / device ---------------------------------------------------- */

/* Bind the calling process to HIP device `device` (one process per GPU).  Must
 * be called before anything else.  Fails with GMG_ENODEV when no GPU or the
 * device is not gfx950 -- there is no CPU fallback. */
int gmg_init(int device);
int gmg_device_count(void);
const char *gmg_last_error(void);
const char *gmg_version(void);
int gmg_synchronize(void *stream);
/* Tuning and test switches (nothing a caller needs for correct results): `key` is one of seg_plain, mg_tile, mg_one_stream,
 * mg_err_flat, mg_err_calls, mg_err_calls_grow, orfs_exact_path, train_sort_min, mg_max_entries, mg_timing, ingest_timing,
 * train_timing, strings_fused, mg_gene32, mg_fused, mg_err_skip, mg_orfs_events, diag.  gmg_init() reads GMG_<KEY IN UPPER CASE> from the
 * environment ONCE; no scoring call reads the environment. */
int gmg_set_option(const char *key, long long value);
int gmg_get_option(const char *key, long long *value);

/* ---- host-side packing helpers (no GPU needed) ---------------------------- */

/* 2-bit code of one character after the reference's load-time normalisation
 * tolower(Filter(ch)) (src/Glimmer/glimmer3.cc:270-271, src/Common/gene.cc:1139-1175)
 * followed by Subscript (src/ICM/icm.cc:2008-2027). */
int gmg_base_code(int ch);
/* Pack n characters starting at job-wide base index `first_base` into `packed`
 * (which must be zero-initialised or already hold the preceding bases). */
int gmg_pack_bases(const char *ascii, uint64_t n, uint64_t first_base, uint32_t *packed);
/* Number of uint32 words needed for total_bases bases (+ one guard word). */
uint64_t gmg_packed_words(uint64_t total_bases);

/* ---- models: replaces ICM_t's table (src/ICM/icm.hh:106-129) -------------- */

/* mip[p*num_nodes+n], prob4[(p*num_nodes+n)*4+b] exactly as ICM_t::Input builds
 * them (src/ICM/icm.cc:614-726) or Build_Indep_WO_Stops (icm.cc:65-216).
 * Supported: model_len <= 32, mut_info_pos in [-2, model_len-1].
 * The fast six-frame kernel additionally needs model_len <= 16, model_depth <= 8;
 * other shapes take the generic kernels (same results). */
int gmg_model_upload(const int16_t *mip, const float *prob4, int model_len, int model_depth,
                     int periodicity, int num_nodes, gmg_model **out);
int gmg_model_free(gmg_model *m);
int gmg_model_info(const gmg_model *m, int *model_len, int *model_depth, int *periodicity,
                   int *num_nodes);

/* ---- a batch of models from the bytes of their .icm files ---------------------- */
/* The six header ints of a binary .icm, validated as ICM_t::Try_Input does (its messages in gmg_last_error(), status
 * GMG_EBADMODEL).  Host only, no device needed.  blob_bytes (may be NULL): the size of the model's device tables; asking for it
 * also applies gmg_model_upload's shape checks. */
int gmg_icm_bytes_info(const void *bytes, uint64_t n_bytes, int *model_len, int *model_depth,
                       int *periodicity, int *num_nodes, uint64_t *blob_bytes);

/* n models in ONE device block, parsed and flattened on the device from the raw bytes of n binary .icm files.
 *   gmg_model_set_load    reads the 24 header bytes of every file on the host (Try_Input's header messages, gmg_model_upload's
 *                         shape checks: GMG_EBADMODEL), then queues on `stream` the copy of all files (a single copy when
 *                         bytes[k+1] == bytes[k] + n_bytes[k] for every k) and the kernels; it does not wait.  bytes[k] must stay
 *                         valid and unchanged until gmg_model_set_finish returns.
 *   gmg_model_set_finish  waits for the stream's work and reads one status word per model.  GMG_EBADMODEL and *bad_file (may be
 *                         NULL; -1 when all are good) for the first file the device refused, Try_Input's / gmg_model_upload's
 *                         message in gmg_last_error().  One refusal is new: a record whose id does not exceed its predecessor's
 *                         inside a sub-model (the reference's writer never produces one; gmg_icm_open reads such a file with the
 *                         last record winning).  A refused set only serves gmg_model_set_free.
 *   gmg_model_set_model   member k, valid after a successful finish; owned by the set -- never gmg_model_free.  It equals
 *                         gmg_icm_open + gmg_icm_device_model on that file byte for byte.
 *   gmg_model_set_free    does not block the host: the block goes back to the library's cache behind the load stream's work and
 *                         whatever the null stream holds at the call; work on any other stream that uses the models must be
 *                         complete.
 * Pattern for a database: load batch k+1 on a second stream, score batch k, finish k+1, free k. */
typedef struct gmg_model_set gmg_model_set;
int gmg_model_set_load(const void *const *bytes, const uint64_t *n_bytes, int n_files,
                       gmg_model_set **out, void *stream);
int gmg_model_set_finish(gmg_model_set *s, int *bad_file);
const gmg_model *gmg_model_set_model(const gmg_model_set *s, int k);
int gmg_model_set_free(gmg_model_set *s);
/* The device tables of a model as one blob, in gmg_model_upload's layout (tests, debugging): with dst NULL only *bytes is set,
 * otherwise *bytes is the room at dst on entry and the blob's size on return. */
int gmg_model_blob(const gmg_model *m, void *dst, size_t *bytes);
/* What the values of a model allow (the smallest and largest exponent field among its non-zero values, whether any is positive,
 * denormal, infinite or a NaN): the figures that choose between the reordered sums and the sequential kernels. */
int gmg_model_value_stats(const gmg_model *m, int *min_exp, int *max_exp, int *odd_values);

/* ---- reads ------------------------------------------------------------------ */

int gmg_reads_upload(const uint32_t *packed2bit, const uint64_t *base_offsets, uint64_t n_reads,
                     gmg_reads **out);
/* Take packed reads that are ALREADY in HBM (e.g. generated on device): one
 * device-to-device copy into the library's guarded buffer; the offsets are used
 * in place and must stay valid until gmg_reads_free.  Neither buffer is freed. */
int gmg_reads_wrap_device(const uint32_t *d_packed2bit, const uint64_t *d_base_offsets,
                          uint64_t n_reads, uint64_t total_bases, gmg_reads **out);
int gmg_reads_free(gmg_reads *r);
int gmg_reads_info(const gmg_reads *r, uint64_t *n_reads, uint64_t *total_bases);
/* Copies the batch back to HOST buffers: packed2bit[gmg_packed_words(total_bases)], base_offsets[n_reads + 1]. */
int gmg_reads_download(const gmg_reads *reads, uint32_t *packed2bit, uint64_t *base_offsets);
/* A new batch made of reads idx[0..n) of `reads` (host indices; any order, repeats allowed), gathered on the device:
 * the grouping step of glimmer-mg's classification mode, where every ICM scores the reads classified to it with the
 * null model of their classes (src/Glimmer/glimmer-mg.cc:361-375, 2050-2068) -- one gmg_mg_score_reads call per group. */
int gmg_reads_select(const gmg_reads *reads, const uint64_t *idx, uint64_t n, gmg_reads **out);

/* ---- regions of reads as a new batch: what build-icm parses back from the text of extract / multi-extract (src/Util/extract.cc,
 * multi-extract.cc), without the text in between; the text itself is gmg_regions_text below ----
 * String k of *out is region k (a gmg_gene_region, declared with the entropy calls below, with the meaning they give it): `len`
 * bases of read `read` from the 0-based `first`, read upwards (strand > 0) or downwards and complemented (strand < 0), positions
 * modulo the read's length; empty regions give empty strings.  first in [0, read length), 0 <= len <= read length, strand != 0,
 * read < n_reads: GMG_ERANGE naming the first bad region otherwise, and nothing is returned.  n = 0 gives a valid empty batch.
 * GMG_EXTRACT_REVERSED: every string comes out back to front (what build-icm -r does to its input), in the same pass.
 * The exceptions: on the reverse strand the reference prints Complement (letter) and the trainer takes Subscript of THAT, which is
 * the code complement only for a c g t d h r y.  amb_base[0 .. n_amb): ascending job-wide base indices, in `reads`, of the bases
 * whose letter is outside acgtACGT; amb_rev_code[i] = Subscript (Complement (letter)) (gmg_fasta_ambiguous makes both).  Where a
 * strand < 0 region covers such a base the string holds amb_rev_code[i]; forward regions are never touched.  n_amb = 0 (NULL
 * pointers): plain code complements.
 * Null stream; returns when the batch is ready (as gmg_reads_select); free it with gmg_reads_free. */
struct gmg_gene_region;
#define GMG_EXTRACT_REVERSED 1
int gmg_reads_extract(const gmg_reads *reads, const struct gmg_gene_region *regions, uint64_t n, int flags,
                      const uint64_t *amb_base, const uint8_t *amb_rev_code, uint64_t n_amb, gmg_reads **out);
/* host only.  Every sequence byte of `bytes` outside acgtACGT: its job-wide base index (as gmg_fasta_ingest numbers the bases)
 * and Subscript (Complement (byte)) (src/Common/gene.cc:15-19, 1084-1091; src/ICM/icm.cc:2008-2027).  cap = room in both arrays;
 * *n = how many there are (call with cap 0 to size); entries beyond cap are counted, not written. */
int gmg_fasta_ambiguous(const char *bytes, uint64_t n_bytes, uint64_t *base, uint8_t *rev_code, uint64_t cap, uint64_t *n);
/* Coordinate lines to regions: the arithmetic of extract (src/Util/extract.cc:84-149) or, with GMG_COORD_MULTI, multi-extract
 * (src/Util/multi-extract.cc:131-173).  A gmg_coord is one parsed line: 1-based inclusive start and end on read `read`; dir is
 * the line's direction field, used under GMG_COORD_USE_DIR (forward when > 0).  Without it a line is forward when
 *   (start < end && (!circular || end - start <= L / 2)) || (circular && start - end > L / 2),   circular = !GMG_COORD_NOWRAP.
 * Length 1 + |end - start| in the line's direction, plus L when negative; extract tests it against min_len before AND after the
 * cuts of GMG_COORD_SKIP_START (3 bases off the start: the start moves up on the forward strand, DOWN on the reverse strand) and
 * GMG_COORD_SKIP_STOP (3 off the end), multi-extract only after them.  A line that fails a test is skipped; a length below 0
 * that passes gives an empty region, as the reference prints an empty record.
 * regions / coord_of_region: room for n entries each (coord_of_region may be NULL); *n_regions of them are written, in the
 * order of the lines, coord_of_region[k] = the line of region k.  base_offsets: the batch's n_reads + 1 offsets (HOST).
 * GMG_ERANGE naming the line: a read index beyond n_reads, an empty sequence, a start that one wrap does not bring into [0, L)
 * (the reference indexes outside its string there), a length above L (the reference walks round the circle again; this
 * library refuses: INTEGRATION.md). */
typedef struct gmg_coord { uint32_t read; int32_t dir; int64_t start, end; } gmg_coord;
#define GMG_COORD_USE_DIR 1     /* extract -d   */
#define GMG_COORD_NOWRAP 2      /* extract -w   */
#define GMG_COORD_SKIP_START 4  /* extract -s   */
#define GMG_COORD_SKIP_STOP 8   /* extract -t   */
#define GMG_COORD_MULTI 16      /* multi-extract's order of the tests */
int gmg_extract_plan(const uint64_t *base_offsets, uint64_t n_reads, const gmg_coord *coords, uint64_t n, int flags,
                     int64_t min_len, struct gmg_gene_region *regions, uint64_t *coord_of_region, uint64_t *n_regions);

/* ---- regions of reads as text: what extract / multi-extract print (src/Util/extract.cc:158-207, multi-extract.cc:215-262) ----
 * The reference prints LETTERS, not codes: seq [i] on the forward strand, Complement (seq [i]) on the reverse strand, so the text
 * is a gather over the sequences' own bytes.  A gmg_letters holds those bytes in HBM, one per base, with the job-wide base
 * numbering of gmg_fasta_ingest: letters[base_offsets[r] .. base_offsets[r + 1]) is read r (the caller compacts the file on the
 * host; base_offsets[0] = 0).  The handle also owns the device buffer the text is written to.
 *
 * gmg_regions_text: record k of the text is, in order, heads[head_off[k] .. head_off[k + 1]) verbatim (HOST arrays; head_off[0] = 0,
 * ascending, a head shorter than 2^32 bytes: GMG_EINVAL otherwise), the letters of region k through params->fwd (strand > 0) or
 * params->rev (strand < 0), with a '\n' in front of a letter whenever params->width letters already stand on the line (width 0:
 * never), and a final '\n': 61 letters at width 60 give 60 '\n' 1 '\n', 60 letters give 60 '\n', no letter gives '\n'.
 * A region is a gmg_gene_region with exactly the meaning gmg_reads_extract gives it (positions modulo the read's length, strand < 0
 * walks downwards), under the same checks -- and a read shorter than 2^31 bases: GMG_ERANGE naming the first bad region
 * otherwise, with nothing written.  n = 0 is valid and gives 0 bytes.
 * *bytes: in, the capacity of host_out; out, the length of the text.  host_out NULL only asks for that length (no device
 * work); a smaller capacity is GMG_ERANGE (*bytes still reports the length, host_out is untouched).  Text offsets are 64-bit.
 * The text is written by k_regions_text on `stream` and copied to host_out; the call synchronises `stream`.
 * gmg_regions_text_device: the same text left on the device: *d_text points into a buffer the handle owns, valid until the
 * next text call on the handle or gmg_letters_free; synchronises `stream` as well.
 * gmg_letters_kernel_ms: the device time of the last call's write kernel, between two events on its stream (0 when it wrote
 * nothing).  One call at a time per handle.
 * gmg_text_params_reference (host only): fwd = every byte itself, rev = the reference's Complement (src/Common/gene.cc:15-19: the
 * IUPAC pairs in either case, blank * - . _ themselves, any other upper-case letter 'N', everything else 'n'). */
typedef struct gmg_letters gmg_letters;
typedef struct gmg_text_params {
    uint8_t fwd[256], rev[256];  /* the byte printed for a letter on the forward / on the reverse strand */
    uint32_t width;              /* letters per line; 0 = all on one line */
    uint32_t reserved;           /* 0 */
} gmg_text_params;
int gmg_letters_upload(const char *letters, const uint64_t *base_offsets, uint64_t n_reads, gmg_letters **out);
int gmg_letters_free(gmg_letters *letters);
int gmg_letters_kernel_ms(const gmg_letters *letters, float *ms);
int gmg_text_params_reference(gmg_text_params *params, uint32_t width);
int gmg_regions_text(gmg_letters *letters, const struct gmg_gene_region *regions, uint64_t n, const char *heads, const uint64_t *head_off,
                     const gmg_text_params *params, char *host_out, size_t *bytes, void *stream);
int gmg_regions_text_device(gmg_letters *letters, const struct gmg_gene_region *regions, uint64_t n, const char *heads,
                            const uint64_t *head_off, const gmg_text_params *params, const char **d_text, size_t *bytes, void *stream);

/* ---- strings spliced from several pieces of a read: scripts/extract_aa.py without the text -------------------------------
 * What glimmer-mg's retraining loop needs under -i / -s: the gene strings with every predicted insertion, deletion and
 * substitution applied to the read (train_features.py --indels = extract_aa.py | build-icm -r).
 *
 * gmg_reads_splice: string k of *out is the concatenation of runs[string_run_off[k] .. string_run_off[k + 1]) (HOST arrays;
 * string_run_off ascends from 0 to n_runs).  A run is `len` bases of read `read` of `reads`:
 *   GMG_RUN_UP        positions first, first + 1, ...                     codes as they are
 *   GMG_RUN_DOWN      positions first, first - 1, ...                     3 - code
 *   GMG_RUN_SUB_UP    as UP, every code replaced by the script's substitution on codes: c -> g, anything else -> c
 *   GMG_RUN_SUB_DOWN  as DOWN, the substitution first, then 3 - code
 *   GMG_RUN_LITERAL + c, GMG_RUN_LITERAL_AS_IS + c (c = 0 .. 3): `len` times the code c; read and first are not looked at (the
 *                     plan leaves the base the literal stands for in them; AS_IS tells a caller that prints letters that the
 *                     letter there is printed as it is -- the script's rc() on a letter outside ATCGatcg)
 * Nothing wraps: an upward run needs first + len <= read length, a downward one len <= first + 1 and first < read length (any
 * first <= read length when len = 0); read < n_reads, kind one of the above: GMG_ERANGE naming the first bad run otherwise, and
 * nothing is returned.  Empty strings and empty runs are fine; n_strings = 0 gives a valid empty batch.
 * GMG_EXTRACT_REVERSED: every string comes out back to front (build-icm -r), in the same pass.
 * Null stream; returns when the batch is ready (as gmg_reads_extract); free it with gmg_reads_free. */
typedef struct gmg_splice_run { uint32_t read, first, len, kind; } gmg_splice_run;
#define GMG_RUN_UP 0
#define GMG_RUN_DOWN 1
#define GMG_RUN_SUB_UP 2
#define GMG_RUN_SUB_DOWN 3
#define GMG_RUN_LITERAL 4
#define GMG_RUN_LITERAL_AS_IS 8
int gmg_reads_splice(const gmg_reads *reads, const gmg_splice_run *runs, uint64_t n_runs, const uint64_t *string_run_off,
                     uint64_t n_strings, int flags, gmg_reads **out);
/* host only.  The edit arithmetic of scripts/extract_aa.py: the gene lines of a predict file to the runs of their strings.
 * genes[0 .. n_genes): the lines in file order (the lines of one read need not be adjacent; their order is what counts): read,
 * the second and third column, the frame column (forward when > 0) and how many I: / D: / S: positions the line lists;
 * positions: those lists back to back -- line 0's insertions, deletions, substitutions, then line 1's -- as written (1-based).
 * odd_base / odd_letter (n_odd may be 0): the ascending job-wide indices of the bases whose letter is not an upper-case A C G T
 * (gmg_fasta_not_upper_acgt) and those letters; with them the runs hold literals where the rules on codes differ from the
 * script's rules on letters (a substitution on any such letter gives C; rc() complements acgt and leaves any other letter).
 * What the script does, restated:
 *   get_preds     the shift of a read, sum of (deletions - insertions listed) over its lines in file order, moves a line's start
 *                 by the sum in front of the line and its end by the sum including it; start = column 2 - 1, end = column 3 on
 *                 the forward strand, start = column 3 - 1, end = column 2 on the reverse strand.  The lines of a read are then
 *                 sorted by start, stably.
 *   predict_msa   one step per base f = 0, 1, ... of the read against the three sorted lists of ALL lines of the read, a cursor
 *                 each; the first of insertion, deletion, substitution whose cursor stands at f wins and only that cursor
 *                 moves (a cursor that is passed -- a position listed twice, or taken by a list of higher priority, or below
 *                 1 -- never moves again; positions beyond the read never fire).  An insertion drops base f.  A deletion
 *                 puts out what the step before put out once more (nothing after a dropped base, a pad blank at f = 0), then
 *                 base f.  A substitution puts out G for the letter C and C for any other letter.  Three pad blanks in front;
 *                 three behind and one more for every listed deletion that did not fire.
 *   print_frag_genes   s counts the corrected characters from -3.  Forward: inside [start, start + 3) the frame restarts and
 *                 the string begins at s = start >= 0; inside [end - 3, end) the walk is switched off; elsewhere, while switched
 *                 on, the string grows once begun, and begins at the first s >= 0 on a codon boundary.  Reverse: [start,
 *                 start + 3) switches the walk on without output, [end - 3, end) switches it off and adds every character that
 *                 is no blank, elsewhere as forward.  The string is cut to a multiple of three characters, blanks counted,
 *                 and a reverse string is then reversed and complemented.
 * Output, room for n_genes entries each: strings[j] for the j-th record the script prints -- reads ascending, the lines of a
 * read by adjusted start -- with the line it came from, start and end as the record name shows them, the strand, and the
 * blanks in front of and behind the printed string (pads never become runs); string_run_off[n_genes + 1]; runs[0 .. *n_runs).
 * runs_cap = room in runs; runs beyond it are counted, not written (call with 0 to size).
 * GMG_ERANGE naming the line: a read index beyond n_reads, a read of 2^31 bases or more. */
typedef struct gmg_edit_gene { uint32_t read; int32_t frame; int64_t col2, col3; uint32_t n_ins, n_del, n_sub, reserved; } gmg_edit_gene;
typedef struct gmg_edit_string { uint64_t gene; int64_t start, end; int32_t strand; uint32_t pad_front, pad_behind, reserved; } gmg_edit_string;
int gmg_edits_plan(const uint64_t *base_offsets, uint64_t n_reads, const gmg_edit_gene *genes, uint64_t n_genes,
                   const int64_t *positions, const uint64_t *odd_base, const char *odd_letter, uint64_t n_odd,
                   gmg_splice_run *runs, uint64_t runs_cap, uint64_t *n_runs, uint64_t *string_run_off, gmg_edit_string *strings);

/* ---- strings of runs as text: the .ffn and .faa files of scripts/extract_aa.py (print_frag_genes, translate) -------------------
 * gmg_runs_text writes, over the letters of a gmg_letters, the strings a plan of runs describes (gmg_edits_plan makes one) or
 * their translations, as gmg_regions_text writes regions: same buffers, same line rule, one kernel (k_runs_text).
 * The printed string P_k of string k is pad_front[k] times params->pad, the bytes of runs[string_run_off[k] ..
 * string_run_off[k + 1]) in order, and pad_behind[k] times params->pad (HOST arrays; NULL pad arrays mean 0; string_run_off
 * ascends from 0 to n_runs: GMG_EINVAL otherwise).  Position i of a run of `len` bytes prints, with x the byte of read `read` of
 * `letters` at the position named:
 *   GMG_RUN_UP                 up[x],       x at first + i
 *   GMG_RUN_DOWN               down[x],     x at first - i
 *   GMG_RUN_SUB_UP             sub_up[x],   x at first + i
 *   GMG_RUN_SUB_DOWN           sub_down[x], x at first - i
 *   GMG_RUN_LITERAL + c        literal[c]; read and first are not looked at
 *   GMG_RUN_LITERAL_AS_IS + c  up[x], x at first, `len` times: here read and first ARE looked at, unlike in gmg_reads_splice
 * The runs obey gmg_reads_splice's rules -- nothing wraps: first + len <= read length upwards, len <= first + 1 and first < read
 * length downwards (any first <= read length when len = 0), read < n_reads, a known kind -- and an AS_IS run with len > 0 needs
 * read < n_reads and first < read length (with len = 0 neither is looked at): GMG_ERANGE naming the first bad run otherwise, with
 * nothing written.  A string of 2^32 characters or more, pads included, is GMG_ERANGE as well.
 * Record k of the text: heads[head_off[k] .. head_off[k + 1]) verbatim (as for gmg_regions_text), the record's characters with a
 * '\n' in front of a character whenever params->width characters already stand on the line (width 0: never), and a final '\n'.
 * The characters are, under GMG_RUNS_TEXT_DNA, the bytes of P_k; under GMG_RUNS_TEXT_PROTEIN, one per whole codon: character t
 * translates P_k[3t .. 3t + 2], t < |P_k| / 3 rounded down (a tail of one or two bytes is dropped): aa[idx] where the three bytes
 * are all upper-case A C G T, aa[idx] with A .. Z lowered (so '*' stays) where they are all lower-case a c g t, and `unknown` for
 * anything else, pad bytes included; idx = 16*b0 + 4*b1 + b2 with a=0 c=1 g=2 t=3, the index of gmg_xlate_table.
 * A mode other than the two, or a non-zero reserved byte, is GMG_EINVAL.
 * host_out, *bytes, n_strings = 0, `stream`, the _device variant and gmg_letters_kernel_ms: exactly as for gmg_regions_text; the
 * text buffer is the handle's one, so a text left on the device is valid until the next text call of EITHER kind on the handle.
 * gmg_runs_text_params_script (host only) fills the script's rules: up = every byte itself, down = the script's rc() on a letter
 * (ATCGatcg swapped, any other byte itself), sub_up = 'G' for 'C' and 'C' for anything else, sub_down = rc() of sub_up, literal =
 * "ACGT", pad = ' ', unknown = 'X', width = 0, and aa = the script's dictionary (the standard code) for transl_table 0, else
 * gmg_xlate_table (transl_table), whose error is passed on. */
#define GMG_RUNS_TEXT_DNA 0
#define GMG_RUNS_TEXT_PROTEIN 1
typedef struct gmg_runs_text_params {
    uint8_t up[256], down[256], sub_up[256], sub_down[256]; /* byte printed for a sequence byte, per kind of run */
    uint8_t literal[4];   /* GMG_RUN_LITERAL + c */
    uint8_t pad;          /* byte of a pad position */
    uint8_t unknown;      /* protein: a codon that is neither all upper-case ACGT nor all lower-case acgt */
    uint8_t reserved[2];  /* 0 */
    char aa[64];          /* protein: index 16*b0 + 4*b1 + b2, a=0 c=1 g=2 t=3, as gmg_xlate_table fills it */
    uint32_t width;       /* characters per line, 0 = one line; the line rule of gmg_regions_text */
    uint32_t mode;
} gmg_runs_text_params;
int gmg_runs_text_params_script(gmg_runs_text_params *params, int mode, int transl_table);
int gmg_runs_text(gmg_letters *letters, const gmg_splice_run *runs, uint64_t n_runs, const uint64_t *string_run_off, uint64_t n_strings,
                  const uint32_t *pad_front, const uint32_t *pad_behind, const char *heads, const uint64_t *head_off,
                  const gmg_runs_text_params *params, char *host_out, size_t *bytes, void *stream);
int gmg_runs_text_device(gmg_letters *letters, const gmg_splice_run *runs, uint64_t n_runs, const uint64_t *string_run_off,
                         uint64_t n_strings, const uint32_t *pad_front, const uint32_t *pad_behind, const char *heads,
                         const uint64_t *head_off, const gmg_runs_text_params *params, const char **d_text, size_t *bytes, void *stream);

/* ---- one string at a time ------------------------------------------------------
 * The ICM_t methods take ONE string per call (src/ICM/icm.hh:131-180).  A gmg_single keeps what such a call needs --
 * page-locked host staging, the packed read, its one segment and a result buffer on the device -- from call to call, so
 * that a call is one copy in, one launch and one copy out (no allocation).  One per host thread; glimmer-mg_amd/host/icm.cc
 * holds one per thread.  gmg_single_stage: the string `ascii` of n characters as a one-read batch with the whole read as
 * its segment in orientation `orient`; *reads / *segs are valid until the next stage call; *d_out has room for n + 16
 * doubles.  gmg_single_fetch copies n_doubles of it back (after the stream's work). */
typedef struct gmg_single gmg_single;
int gmg_single_create(gmg_single **out);
int gmg_single_stage(gmg_single *st, const char *ascii, uint64_t n, int orient, const gmg_reads **reads,
                     const gmg_segments **segs, double **d_out);
int gmg_single_fetch(gmg_single *st, double *dst, size_t n_doubles);
int gmg_single_free(gmg_single *st);
/* ICM_t::Full_Window_Prob / Full_Window_Distrib (src/ICM/icm.cc:512-610) for ONE window of model_len codes (0..3, one byte each)
 * under sub-model `frame`, on the staging of st: dist4 (4 floats, may be NULL), prob (may be NULL). */
int gmg_single_window(gmg_single *st, const gmg_model *m, const uint8_t *codes, int model_len, int frame, float *dist4, double *prob);

/* ---- segments --------------------------------------------------------------- */

/* Validates every segment against the read lengths (GMG_ERANGE otherwise).
 * out_total_len receives sum(len); per-position outputs of segment i start at
 * the exclusive prefix sum of the lengths (also returned in out_offsets if not NULL,
 * n_segments+1 entries). */
int gmg_segments_upload(const gmg_reads *reads, const gmg_segment *segs, uint64_t n_segments,
                        uint64_t *out_offsets, uint64_t *out_total_len, gmg_segments **out);
int gmg_segments_free(gmg_segments *s);

/* ---- scoring ---------------------------------------------------------------- */

/* Six-frame per-position scores of whole reads: replaces Score_All_Frames
 * (src/Glimmer/glimmer-mg.cc:1468-1510), i.e. 12 x ICM_t::Frame_Score
 * (src/ICM/icm.cc:485-509) + the gene - null subtraction in double.
 *   d_out[f*total_bases + base_offsets[r] + p],  f = 0..5, p = 0..len(r)-1
 * equals Frame_Scores[f][p] of read r bit for bit.  Both models need periodicity
 * >= 3 (Frame_Score asserts frame < periodicity, src/ICM/icm.cc:496); `null_model`
 * normally is the (3,2,3) Build_Indep_WO_Stops model. */
int gmg_frame_score6(const gmg_model *gene, const gmg_model *null_model, const gmg_reads *reads,
                     double *d_out, void *stream);
/* The same table with its six rows row_stride (>= total_bases) doubles apart:
 *   d_out[f*row_stride + base_offsets[r] + p].
 * The kernel stores two doubles per lane when every row starts on a 16-byte boundary (d_out 16-byte aligned and
 * row_stride even), one at a time otherwise (about 15% slower); a batch of ragged reads has an odd total_bases half of
 * the time, so a caller that owns the table should round the stride up (gmg_mg_score_reads does for its own table). */
int gmg_frame_score6_strided(const gmg_model *gene, const gmg_model *null_model, const gmg_reads *reads,
                             double *d_out, uint64_t row_stride, void *stream);

/* Per-read null models: a set of (3,2,3) Build_Indep_WO_Stops models on the device (1 KB each), and the six-frame table
 * with read r scored against null model read_null[r] (HOST array, n_reads entries) -- what Score_All_Frames gives inside
 * glimmer-mg's classification loop, where Update_Meta_Null_ICM (glimmer-mg.cc:2050-2068) rebuilds Indep_Model per read.
 * (Two passes: fp32 gene values, then the null model's part; gmg_mg_score_reads with gmg_mg_params.nulls applies the
 * null models where it builds its running sums, at no extra pass.) */
typedef struct gmg_null_set gmg_null_set;
int gmg_null_set_upload(const gmg_model *const *null_models, int n_models, gmg_null_set **out);
/* The same set from HOST tables: mip[n][3][21], prob4[n][3][21][4] as Build_Indep_WO_Stops fills (3,2,3) models; one copy. */
int gmg_null_set_from_tables(const int16_t *mip, const float *prob4, int n_models, gmg_null_set **out);
/* ... or from the GC values themselves: model i = Build_Indep_WO_Stops (gc_frac[i], stop_codon) (src/ICM/icm.cc:65-216,
 * the library's host ICM_t) -- what Update_Meta_Null_ICM (glimmer-mg.cc:2050-2068) builds per read. */
int gmg_null_set_build(const double *gc_frac, int n_models, const char (*stop_codon)[4], int n_stop_codons,
                       gmg_null_set **out);
int gmg_null_set_free(gmg_null_set *nulls);
int gmg_frame_score6_nulls(const gmg_model *gene, const gmg_null_set *nulls, const uint32_t *read_null,
                           const gmg_reads *reads, double *d_out, uint64_t row_stride, void *stream);

/* ICM_t::Frame_Score (src/ICM/icm.cc:485-509) on every segment: one fixed
 * sub-model `frame` for all positions, no sum.  d_out[offset(i)+j]. */
int gmg_segment_frame_score(const gmg_model *m, const gmg_reads *reads, const gmg_segments *segs,
                            int frame, double *d_out, void *stream);

/* ICM_t::Cumulative_Score (src/ICM/icm.cc:354-405) on every segment: running
 * double sum in reference order, sub-model of base 0 = frame0, cycling.
 * This is what Score_Orfs calls twice per ORF (src/Glimmer/glimmer3.cc:1346-1347). */
int gmg_segment_cumscore(const gmg_model *m, const gmg_reads *reads, const gmg_segments *segs,
                         int frame0, double *d_out, void *stream);

/* ICM_t::Score_String (src/ICM/icm.cc:864-903) on every segment: d_sums[i]. */
int gmg_score_string(const gmg_model *m, const gmg_reads *reads, const gmg_segments *segs,
                     int frame0, double *d_sums, void *stream);

/* Whole-read ICM_t::Score_String (src/ICM/icm.cc:864-903, frame 0) of every read AND of its reverse complement
 * under each of n_models models -- what Phymm's scoreReadsGlim.pl asks of `simple-score` for every genome's ICM
 * (scripts/scoreReadsGlim.pl:450,482; BASELINE configs[3]).  d_sums (device): [n_models][n_reads][2] doubles,
 * [..][0] = the read, [..][1] = its reverse complement.  Periodicity-1 models of the default shape (depth 7,
 * window <= 15) take a batched path at the six-frame kernel's rate; any other model goes through the exact
 * segment kernel.  Sums are sequential double additions in string order (bit-identical to the reference). */
int gmg_score_reads_strings(const gmg_model *const *models, int n_models, const gmg_reads *reads,
                            double *d_sums, void *stream);

/* ICM_t::Partial_Window_Prob (src/ICM/icm.cc:807-842) for the LAST base of every
 * segment (predict_pos = len-1), with the partial-window rule applied whatever
 * the length, as the reference does.  d_out[i]; 0.0 for an empty segment. */
int gmg_segment_partial_prob(const gmg_model *m, const gmg_reads *reads, const gmg_segments *segs,
                             int frame, double *d_out, void *stream);

/* All_Frame_Score (src/Glimmer/glimmer3.cc:328-359) on every segment: the
 * segment is the ORF buffer orientation used by Score_Orfs, `d_prefix_len[i]`
 * (device, uint32) is the number of leading buffer bases to score (best_j-2),
 * `d_frame[i]` (device, int32 in {1,2,3,-1,-2,-3}) selects Permute_By_Frame
 * (glimmer3.cc:1013-1088).  d_af[6*i + k]. */
int gmg_all_frame_score(const gmg_model *gene, const gmg_reads *reads, const gmg_segments *segs,
                        const uint32_t *d_prefix_len, const int32_t *d_frame, double *d_af,
                        void *stream);

/* ICM_t::Full_Window_Prob / Full_Window_Distrib (src/ICM/icm.cc:512-610) on
 * n_windows explicit windows.  d_windows: model_len codes (0..3) per window, one
 * byte each; d_frames: sub-model per window.  d_dist4[4*i+b] (may be NULL),
 * d_prob[i] (may be NULL) = (double) dist[code of last window char]. */
int gmg_window_distrib(const gmg_model *m, const uint8_t *d_windows, const int32_t *d_frames,
                       uint64_t n_windows, float *d_dist4, double *d_prob, void *stream);

/* ---- fixed-length ICMs: replaces Fixed_Length_ICM_t's scoring (src/ICM/icm.hh:216-255, icm.cc:1466-1645) -------------
 * A fixed-length model of length L (1 <= L <= 32) is L sub-models; sub-model i (0-based) is an ICM_t of model_len i+1,
 * periodicity 1, that predicts base i of the PERMUTED window from bases 0..i-1 of it.  gmg_fixed_model_upload takes the
 * tables of sub-model i as gmg_model_upload would (mip[i][num_nodes[i]], prob4[i][num_nodes[i] * 4], depth model_depth[i]
 * in [0, min(i, 12)]) and perm[L], which must be a bijection of 0..L-1 (GMG_EBADMODEL otherwise: the reference does not
 * check, an invalid permutation is undefined behaviour there). */
typedef struct gmg_fixed_model gmg_fixed_model;
int gmg_fixed_model_upload(int length, const int32_t *perm, const int16_t *const *mip, const float *const *prob4,
                           const int *model_depth, const int *num_nodes, gmg_fixed_model **out);
int gmg_fixed_model_free(gmg_fixed_model *m);
/* length, the largest sub-model depth and the bytes of the flattened tables on the device (any pointer may be NULL) */
int gmg_fixed_model_info(const gmg_fixed_model *m, int *length, int *max_depth, uint64_t *table_bytes);
/* Fixed_Length_ICM_t::subrange_score (src/ICM/icm.cc:1565-1645) of every segment:
 *   d_out[k] = sum_{i=lo}^{hi-1} FWP_i(perm(B_k[0..L)))
 * with B_k the segment's buffer in its gmg_orient, P = perm(B) the window Permute_String makes (P[i] = B[perm[i]]) and FWP_i
 * ICM_t::Full_Window_Prob of sub-model i on P[0..i].  The sum is double additions in i order from 0.0, as the reference's.
 * Bases of a segment past L are ignored (strncpy (buff, w, length)); a segment shorter than L is GMG_ERANGE; lo == hi
 * gives 0.0; 0 <= lo <= hi <= L (GMG_EINVAL otherwise).  Fixed_Length_ICM_t::Score_Window is lo = 0, hi = L. */
int gmg_fixed_score(const gmg_fixed_model *m, const gmg_reads *reads, const gmg_segments *segs,
                    int lo, int hi, double *d_out, void *stream);

/* ---- Score_Orfs inner loop (src/Glimmer/glimmer3.cc:1275-1552) ------------------- */

/* One Orf_t as Find_Orfs produced it (src/Common/gene.hh:101-139). */
typedef struct gmg_orf {
    uint32_t read;           /* index into the gmg_reads batch                                   */
    int32_t frame;           /* Orf_t::Get_Frame(): +1..+3 forward, -1..-3 reverse                */
    int32_t stop_position;   /* Orf_t::Get_Stop_Position(): first base of the stop codon, 1-based */
    int32_t orf_len;         /* Orf_t::Get_Orf_Len()                                              */
} gmg_orf;

/* The globals Score_Orfs reads (glimmer3.cc:23,61,71,122,148; glimmer_base.cc:2636-2712). */
typedef struct gmg_orf_params {
    int32_t min_gene_len;        /* Min_Gene_Len (default 75)                                    */
    int32_t allow_truncated;     /* Allow_Truncated_Orfs (-X)                                    */
    int32_t use_first_start;     /* Use_First_Start_Codon (-f)                                   */
    int32_t ignore_score_len;    /* Ignore_Score_Len (INT_MAX = never)                           */
    double start_threshold;      /* Start_Threshold (-6)                                         */
    int32_t n_start_codons;      /* <= 8                                                         */
    char start_codon[8][4];      /* Start_Codon strings, e.g. "atg","gtg","ttg" (IUPAC allowed)  */
} gmg_orf_params;

/* One Start_t (src/Glimmer/glimmer_base.hh:80-88), in the order Score_Orfs pushes them. */
typedef struct gmg_start {
    double score;            /* score[j-1] - indep_score[j-1], after the Ignore_Score_Len boost  */
    int32_t j, pos;
    int32_t which;           /* index of the matching start codon, -1 for a truncated start      */
    int16_t truncated, first;
} gmg_start;

typedef struct gmg_orf_result {
    double gene_score;       /* 100 * best_score / (best_j - 2)                  (glimmer3.cc:1489) */
    double best_score;
    uint32_t start_begin;    /* first entry of this ORF's start list in the starts array          */
    uint32_t n_starts;
    int32_t first_j, best_j; /* gene length = best_j + 1                         (glimmer3.cc:1499) */
    int32_t best_pos;
    int16_t is_tentative_gene;   /* first_j+1 >= Min_Gene_Len && best_score > Start_Threshold (:1468); only then
                                    does the reference add the gene and its events (:1494-1548)   */
    int16_t orf_is_truncated;
} gmg_orf_result;

typedef struct gmg_orf_batch gmg_orf_batch;

/* Validates the ORFs against their reads (linear sequences only: the reference's circular wrap-around
 * is refused with GMG_ERANGE) and reserves room for the start lists; *out_max_starts is the number
 * of gmg_start entries the caller must provide to gmg_score_orfs. */
int gmg_orfs_upload(const gmg_reads *reads, const gmg_orf *orfs, uint64_t n_orfs,
                    uint64_t *out_max_starts, gmg_orf_batch **out);
int gmg_orf_batch_free(gmg_orf_batch *b);

/* The scoring part of Score_Orfs for every ORF of the batch: ORF buffer (Reverse_Transfer /
 * Complement_Transfer), gene and null Cumulative_Score from frame 1, the start-codon scan from the
 * 3' end, first/best start, truncated starts, gene score and the tentative-gene test.  `results`
 * (n_orfs) and `starts` (room for out_max_starts entries) are HOST buffers.  The start lists are packed
 * back to back in ORF order on the device, so only sum(n_starts) entries are copied into `starts`
 * (typically ~5 % of out_max_starts); results[i].start_begin indexes that packed array.
 * Events / DP / trace-back stay host code (src/Glimmer/glimmer_base.cc). */
int gmg_score_orfs(const gmg_model *gene, const gmg_model *null_model, const gmg_reads *reads,
                   const gmg_orf_batch *orfs, const gmg_orf_params *params,
                   gmg_orf_result *results, gmg_start *starts, void *stream);

/* The same in two steps, for callers that do not want to reserve out_max_starts entries on the host (a slot per in-frame codon
 * of every ORF: ~100 per ORF, of which ~3 % are used): gmg_score_orfs_begin scores and leaves the results on the device,
 * *out_n_starts = the number of starts of all ORFs; gmg_score_orfs_fetch copies results[n_orfs] and starts[*out_n_starts].
 * The results are complete when gmg_score_orfs_begin returns: the fetch may use any stream. */
int gmg_score_orfs_begin(const gmg_model *gene, const gmg_model *null_model, const gmg_reads *reads,
                         const gmg_orf_batch *orfs, const gmg_orf_params *params, uint64_t *out_n_starts, void *stream);
int gmg_score_orfs_fetch(const gmg_orf_batch *orfs, gmg_orf_result *results, gmg_start *starts, void *stream);

/* ---- glimmer-mg front half on the device -------------------------------------------
 * Everything between the reads and Add_Events_* for glimmer-mg's user-ICM mode (the -i / -s error branch: see the flags below):
 *   Score_All_Frames      src/Glimmer/glimmer-mg.cc:1468-1510   (gmg_frame_score6's kernels)
 *   Find_Orfs             src/Glimmer/glimmer_base.cc:638-779   (linear sequences, no ignore regions)
 *   Save_Prev_Stops       src/Glimmer/glimmer-mg.cc:675-729     (folded into the ORF scan: lo / hi per ORF)
 *   Score_Orf_Starts      src/Glimmer/glimmer-mg.cc:1693-1861   with Cumulative_Frame_Score :561-604
 *   Score_Orfs_Errors     src/Glimmer/glimmer-mg.cc:1632-1685   boost, first_j, best score, threshold
 * The 48 B/base Frame_Scores table never leaves HBM; what comes back is one record per ORF and the start
 * lists.  The caller sorts each accepted ORF's list with Start_Cmp (glimmer_base.hh:90) and hands it to
 * Add_Events_Fwd / Add_Events_Rev exactly as Score_Orfs_Errors does. */
/* gmg_mg_params.flags: return only the ORFs Score_Orfs_Errors would hand to Add_Events_* (accepted != 0) and their start
 * lists -- same order, packed on the device, read_orf_off counting the kept ORFs; typically a few per cent of all ORFs */
#define GMG_MG_ACCEPTED_ONLY 1
/* glimmer-mg's error branch (src/Glimmer/glimmer-mg.cc:1513-1602 Score_Indels, :1771-1806 the substitution branch of
 * Score_Orf_Starts; exclusive, :952): Find_Orfs also keeps every ORF of orf_len >= Min_Indel_ORF_Len
 * (glimmer_base.cc:494,528,806), Score_Orf_Starts recurses through frame shifts at low-quality bases (-i) or through
 * the previous stop codon (-s), and every start carries the Error_t list of its path (gmg_mg_result_fetch_errors). */
#define GMG_MG_ALLOW_INDELS 2    /* glimmer-mg -i / --indel */
#define GMG_MG_ALLOW_SUBS 4      /* glimmer-mg -s / --sub   */

typedef struct gmg_mg_params {
    int32_t min_gene_len;        /* Min_Gene_Len (>= 4)                                           */
    int32_t allow_truncated;     /* Allow_Truncated_Orfs (glimmer-mg default: true)               */
    int32_t ignore_score_len;    /* Ignore_Score_Len                                              */
    int32_t n_start_codons;      /* <= 8                                                          */
    int32_t n_stop_codons;       /* <= 8                                                          */
    int32_t flags;               /* GMG_MG_ACCEPTED_ONLY | GMG_MG_ALLOW_INDELS or GMG_MG_ALLOW_SUBS, or 0 */
    double start_threshold;      /* Start_Threshold                                               */
    char start_codon[8][4];      /* Start_Codon strings (IUPAC allowed)                           */
    char stop_codon[8][4];       /* Stop_Codon strings                                            */
    /* the error branch; read only when flags has GMG_MG_ALLOW_INDELS or GMG_MG_ALLOW_SUBS */
    int32_t min_indel_orf_len;   /* Min_Indel_ORF_Len (glimmer_base.cc:40: 15)                    */
    int32_t indel_quality_threshold;     /* Indel_Quality_Threshold (glimmer-mg.cc:136: 18)       */
    int32_t indel_max;           /* Indel_Max (glimmer-mg.cc:138: 2); 0..2                        */
    int32_t circular;            /* gmg_find_orfs only: Genome_Is_Circular (glimmer-mg -r): every sequence of the batch is circular
                                    (glimmer_base.cc:680-688, Wrap_Around_Back :2793-2850, Wrap_Through_Front :2854-2900)   */
    double indel_suffix_score_threshold; /* Indel_Suffix_Score_Threshold (glimmer-mg.cc:134: -12) */
    const uint8_t *quality;      /* HOST, one Phred value per base, reads back to back (total_bases): the user's quality
                                    file (-q), Clean_Quality_454 (glimmer-mg.cc:519-546) is applied on the device;
                                    NULL: Set_Quality_454 (:1865-1906, homopolymer runs).  Indels only: with -s the
                                    reference never loads the values (:384-392)                    */
    /* classification mode: glimmer-mg rebuilds Indep_Model and Ignore_Score_Len for EVERY read from the GC of its classes
     * (Update_Meta_Null_ICM, glimmer-mg.cc:2050-2068, inside the ICM-grouped loop :361-451).  One call scores a whole
     * ICM group: read r takes model read_null[r] of `nulls` (instead of the null_model argument) and
     * read_ignore_score_len[r] (instead of ignore_score_len above).  All three NULL: one null model for the batch. */
    const struct gmg_null_set *nulls;
    const uint32_t *read_null;           /* HOST [n_reads] */
    const int32_t *read_ignore_score_len;/* HOST [n_reads], or NULL with nulls set: ignore_score_len for every read */
    /* gmg_find_orfs only: glimmer3 -i, Ignore_Region as Get_Ignore_Regions leaves it (glimmer_base.cc:833-930): 0-based lo, hi one past
     * the last ignored base, sorted, overlaps merged; the same regions apply to EVERY sequence of the batch (:844-847) */
    int32_t n_ignore_regions;
    int32_t reserved2;
    const int32_t *ignore_lo, *ignore_hi;        /* HOST [n_ignore_regions] */
} gmg_mg_params;

/* the Error_t list (src/Common/gene.hh:138-146) of one start: type 0 insertion, 1 deletion, 2 substitution */
typedef struct gmg_start_errors {
    int32_t pos[2];
    int8_t type[2];
    int8_t n;                    /* 0..2 entries                                                  */
    int8_t reserved;
} gmg_start_errors;

typedef struct gmg_mg_orf {
    uint32_t read;               /* index into the gmg_reads batch                                */
    int32_t frame, stop_position, orf_len, gene_len;     /* the Orf_t Find_Orfs built             */
    int32_t lo, hi;              /* Score_Orf_Starts' bounds (glimmer-mg.cc:1730-1757)            */
    int32_t first_j;             /* j of the first start (after the sort: front / back)           */
    uint32_t start_begin, n_starts;      /* its start list: starts[start_begin .. +n_starts), in the
                                            order Score_Orf_Starts pushed them, boost applied      */
    int16_t accepted;            /* non-empty, first_j+1 >= Min_Gene_Len, best_score > Start_Threshold
                                    (glimmer-mg.cc:1656-1676): the ORF goes to Add_Events_*.  Error branch only: paths
                                    tie on pos with different j, so first_j is whichever entry the reference's unstable
                                    sort puts first (reported: the smallest).  2 = best_score passes but only some of those
                                    entries pass the length test, so the caller decides after ITS sort -- a guard: the
                                    reference's own filter (glimmer-mg.cc:1821) already makes every pushed j pass */
    int16_t orf_is_truncated;
    int32_t reserved;
    double best_score;           /* max over the boosted start scores, -DBL_MAX if none           */
} gmg_mg_orf;

typedef struct gmg_mg_result gmg_mg_result;

/* Runs the whole front half for every read of the batch.  d_frame_scores: device buffer of
 * 6 * total_bases doubles that receives the Frame_Scores table (the caller may want it), or NULL to let
 * the call allocate and release its own.  Needs a gene model of periodicity 3. */
int gmg_mg_score_reads(const gmg_model *gene, const gmg_model *null_model, const gmg_reads *reads,
                       const gmg_mg_params *params, double *d_frame_scores, gmg_mg_result **out,
                       void *stream);
/* The same for a batch whose reads come in consecutive GROUPS, every group under its own gene ICM: one chunk of glimmer-mg's
 * classification mode (the loop over ICM_Sequences, src/Glimmer/glimmer-mg.cc:361-451: Gene_ICM.Read per group, then every read
 * of the group against the null model and Ignore_Score_Len of ITS classes, Update_Meta_Null_ICM :2050-2068) in ONE call: the
 * reads gathered in visiting order (gmg_reads_select on the order of gmg_classes_plan), groups[k] = reads [read_begin, read_end)
 * of that batch (consecutive, from 0 to n_reads), params->nulls / read_null / read_ignore_score_len per read (required; one
 * stop-codon set per call).  The six-frame pass swaps the group's tables in LDS as it crosses from group to group -- one launch
 * whatever the number of groups (up to 2^27 - 1: a chunk may meet one ICM file per read); everything behind it never sees a gene
 * model.  Results as gmg_mg_score_reads', reads in batch order. */
typedef struct gmg_mg_group {
    const gmg_model *gene;
    uint64_t read_begin, read_end;
} gmg_mg_group;
int gmg_mg_score_groups(const gmg_mg_group *groups, int n_groups, const gmg_model *null_model, const gmg_reads *reads,
                        const gmg_mg_params *params, gmg_mg_result **out, void *stream);
/* Find_Orfs alone (src/Glimmer/glimmer_base.cc:638-817) for every read of the batch -- the ORF list glimmer3's Score_Orfs /
 * gmg_score_orfs and glimmer-mg's Score_Orfs_Errors start from.  Uses min_gene_len, allow_truncated and the codon lists of
 * `params`; the result holds the Orf_t fields (and lo / hi), no start lists (n_starts = 0).  With params->n_ignore_regions
 * (glimmer3 -i) or params->circular (glimmer-mg -r) the scan follows the reference's other two modes (lo = hi = 0 then);
 * GMG_EINVAL where the reference itself aborts (a circular sequence with a reverse frame that holds no stop codon). */
int gmg_find_orfs(const gmg_reads *reads, const gmg_mg_params *params, gmg_mg_result **out, void *stream);
/* Sizes of the result: ORFs of all reads (Find_Orfs order, read by read) and start entries. */
int gmg_mg_result_info(const gmg_mg_result *r, uint64_t *n_orfs, uint64_t *n_starts);
/* Copies the result to HOST buffers: orfs[n_orfs], starts[n_starts] and, if not NULL,
 * read_orf_off[n_reads + 1] (ORFs of read i are orfs[read_orf_off[i] .. read_orf_off[i+1])). */
int gmg_mg_result_fetch(const gmg_mg_result *r, gmg_mg_orf *orfs, gmg_start *starts, uint64_t *read_orf_off);
/* Error branch: errs[n_starts], parallel to starts (all-zero entries without the error flags); copied on the stream the scoring
 * call ran on, which must still exist. */
int gmg_mg_result_fetch_errors(const gmg_mg_result *r, gmg_start_errors *errs);
/* the same copies on `stream` (they then overlap the scoring of the next batch on another stream) */
int gmg_mg_result_fetch_on(const gmg_mg_result *r, gmg_mg_orf *orfs, gmg_start *starts, uint64_t *read_orf_off,
                           void *stream);
int gmg_mg_result_free(gmg_mg_result *r);
/* gmg_mg_* keeps released device buffers for the next call (allocation of GB-sized buffers is slow);
 * this returns the idle ones to the driver. */
int gmg_trim_cache(void);
/* tests, debugging: the device blocks that the library's handles hold straight from hipMalloc, not from that cache (models, null
 * sets, gmg_single, ORF batches, top hits, fixed models) -- a process-wide count; a handle that is freed holds none. */
int gmg_debug_owned_blocks(uint64_t *out);

/* ---- FASTA ingest on the device -----------------------------------------------------
 * Replaces the loop  while (Fasta_Read (fp, seq, hdr))  (src/Common/fasta.cc:236-286) + the per-base
 * tolower (Filter (ch)) of the callers (src/Glimmer/glimmer3.cc:270-271, glimmer-mg.cc:381-382) + the g/c count of
 * Set_GC_Fraction (src/Glimmer/glimmer_base.cc:2564-2595).  `bytes` is the whole file (host memory, < 2^31 bytes);
 * it is copied to the device once and parsed there.  Records follow Fasta_Read exactly: a '>' anywhere outside a
 * header line starts a record, the header runs to the end of that line, every non-isspace byte up to the next '>'
 * is a base, bytes in front of the first '>' are skipped.  *reads is ready for every scoring call;
 * *index keeps the counts and, per read, the extent of its header line in `bytes`. */
typedef struct gmg_fasta gmg_fasta;
int gmg_fasta_ingest(const char *bytes, uint64_t n_bytes, gmg_reads **reads, gmg_fasta **index);
/* the same, with every copy and kernel on `stream` (a pipeline ingests piece i+1 while piece i is scored) */
int gmg_fasta_ingest_on(const char *bytes, uint64_t n_bytes, gmg_reads **reads, gmg_fasta **index, void *stream);
/* Places where a big file can be cut into pieces of about chunk_bytes for separate gmg_fasta_ingest calls: a '>' that
 * directly follows a newline always starts a record.  cuts[0] = 0 ... cuts[pieces] = n_bytes; returns the number of pieces
 * (at most max_pieces; cuts needs max_pieces + 1 entries). */
int gmg_fasta_split(const char *bytes, uint64_t n_bytes, uint64_t chunk_bytes, uint64_t *cuts, int max_pieces);
/* n_reads, bases of all reads, and how many of them are g or c after filtering (Indep_GC_Frac = gc / total) */
int gmg_fasta_info(const gmg_fasta *index, uint64_t *n_reads, uint64_t *total_bases, uint64_t *gc_count);
/* hdr string of read i = bytes[hdr_begin[i] .. hdr_end[i])  (HOST arrays of n_reads entries) */
int gmg_fasta_headers(const gmg_fasta *index, uint64_t *hdr_begin, uint64_t *hdr_end);
int gmg_fasta_free(gmg_fasta *index);

/* ---- one job over several GPUs / several batches (host only) -----------------------------------
 * Reads shard embarrassingly: every sequence is scored on its own (src/Glimmer/glimmer3.cc:262-310,
 * glimmer-mg.cc:361-451); the one run-wide quantity is the null model's GC fraction, a ratio of two counts over all
 * bases (Set_GC_Fraction, src/Glimmer/glimmer_base.cc:2564-2595).  One process per GPU takes a contiguous range of
 * reads of about equal BASE count, the per-shard {gc, total} counts are summed on the host, results are concatenated
 * in shard order; inside a shard the same plan cuts batches that fit the 32-bit fields of the result records. */
/* read_begin[k] .. read_begin[k+1] = reads of shard k (n_shards + 1 entries); cut k at the read boundary nearest to
 * k * total_bases / n_shards. */
int gmg_shard_plan(const uint64_t *base_offsets, uint64_t n_reads, int n_shards, uint64_t *read_begin);
/* The same on the bytes of an unparsed FASTA file: cuts[k] = the first certain record start ('>' behind a newline) at
 * or behind k * n_bytes / n_shards; cuts[0] = 0, cuts[n_shards] = n_bytes.  Every shard is a valid input of
 * gmg_fasta_ingest / gmg_fasta_split. */
int gmg_fasta_shard_ranges(const char *bytes, uint64_t n_bytes, int n_shards, uint64_t *cuts);
/* Indep_GC_Frac from per-shard counts (gmg_fasta_info).  as_reference != 0: the reference's `unsigned int` counters,
 * which wrap beyond 2^32 bases (byte-identical output on such files); 0: 64-bit counts. */
double gmg_gc_fraction(const uint64_t *gc_counts, const uint64_t *base_counts, int n_shards, int as_reference);

/* ---- glimmer-mg's classification mode, -c (host only) --------------------------------------------
 * With -c every read is scored by the gene ICM its Phymm classes name, against a null model and with stop codons that
 * are rebuilt per read, and the reads are visited -- and <tag>.predict is written -- ICM by ICM in the iteration order of
 * the reference's hash tables, not in file order.  gmg_classes_* reproduce that bookkeeping; the scoring of one ICM's
 * reads is then ONE gmg_mg_score_reads call (gmg_reads_select, gmg_null_set_upload, gmg_mg_params.read_null /
 * read_ignore_score_len) per stop-codon set.  INTEGRATION.md shows the loop; integration/glimmer-mg_gpu.cc runs it. */
typedef struct gmg_classes gmg_classes;
/* Parse_Classes (src/Glimmer/glimmer-mg.cc:726-758) on the text of a classification file ("<read> <class> <class> ..."
 * per line, class = <strain>|<NC>), then Read_Meta_ICMs (:998-1027) with Classes_ICM_File (:473-515; looks for the
 * double ICMs under icm_dir with stat), Read_Meta_GC (:1389-1420: <icm_dir>/<strain>/<NC>.gc.txt, 0.5 when missing) and
 * Read_Meta_Stops (:1211-1250: transl_table of <NC>.gbk, 11 when missing).  icm_dir is the reference's ICM_dir (:147). */
int gmg_classes_load(const char *class_text, uint64_t n_bytes, const char *icm_dir, gmg_classes **out);
int gmg_classes_free(gmg_classes *c);
/* classified reads, distinct ICM files, distinct classes, classes without a .gc.txt (any pointer may be NULL) */
int gmg_classes_info(const gmg_classes *c, uint64_t *n_reads, uint32_t *n_icms, uint32_t *n_classes, uint64_t *n_missing_gc);
/* ICM file k (0 .. n_icms-1) in the order the reference's loop over ICM_Sequences loads them (glimmer-mg.cc:361-364) */
const char *gmg_classes_icm_file(const gmg_classes *c, uint32_t k);
/* The plan of ONE chunk of the input (the reference reads Chunk_Sequences = 500000 reads at a time, glimmer-mg.cc:128,
 * 326-356): hdr[i] / hdr_len[i] = header line of read i of the chunk (its first white-space-delimited token is the key;
 * when two reads share a key the later one is taken, as Read_Indexes does).  order[k], k < *n_order <= n: chunk index of
 * the k-th read the reference processes and prints; order[icm_begin[f] .. icm_begin[f+1]) are the reads of ICM file f
 * (icm_begin: n_icms + 1 entries).  Reads without a line in the class file are never processed (:369-371).  Per
 * processed read, parallel to order (either may be NULL): gc[k] = Indep_GC_Frac of Update_Meta_Null_ICM (:2050-2064: the
 * float GCs of its classes summed in double, divided by their float count), transl[k] = Genbank_Xlate_Code of
 * Update_Meta_Stop (:2196: the table of its FIRST class). */
int gmg_classes_plan(const gmg_classes *c, const char *const *hdr, const uint32_t *hdr_len, uint64_t n,
                     uint64_t *order, uint64_t *icm_begin, double *gc, int32_t *transl, uint64_t *n_order);
/* Set_Stop_Codons_By_Code (src/Common/gene.cc:1560-1624): the stop codons of a GenBank translation table, in the
 * reference's order (Build_Indep_WO_Stops depends on it); GMG_EINVAL for a table the reference does not know. */
int gmg_stop_codons_by_code(int code, char stop_codon[8][4], int *n_stop_codons);
/* Set_Ignore_Score_Len (src/Glimmer/glimmer_base.cc:2597-2633) */
int gmg_ignore_score_len(double gc_frac, const char (*stop_codon)[4], int n_stop_codons, int32_t *out);
/* Codon_Translation (src/Common/gene.cc:1016-1080) as a table: aa[16*b0 + 4*b1 + b2] (base code a=0 c=1 g=2 t=3) = the amino-acid
 * letter of the codon, '*' for a stop, under GenBank translation table `code` -- 0, 1 and 11 (one table), 2, 3, 4, 5, 6, 9, 10, 12,
 * 13, 14, 15, 16, 21, 22, 23; GMG_EINVAL for any other. */
int gmg_xlate_table(int code, char aa[64]);

/* ---- the entropy distance ratio of an ORF (long-orfs -t, glimmer3 -E) ------------------------------------------------------
 * Entropy_Distance_Ratio (src/Glimmer/long-orfs.cc:301-351, the same body in src/Glimmer/glimmer3.cc:423-473): the codons of a
 * region are translated (Codon_Translation, src/Common/gene.cc:1016-1080), the 20 amino-acid counts become an entropy profile
 * (Counts_To_Entropy_Profile, gene.cc:1095-1135) and the ratio is its Euclidean distance to the profile of genes over that to the
 * profile of non-genes.
 * A region is `len` bases of read `read` from the 0-based index `first`: read upwards (strand > 0, Forward_Strand_Transfer,
 * gene.cc:1237-1260) or downwards and complemented (strand < 0, Reverse_Strand_Transfer, gene.cc:1533-1556), both modulo the
 * read's length.  A trailing partial codon, '*' and every letter outside A C D E F G H I K L M N P Q R S T V W Y count nowhere.
 * `aa` is a gmg_xlate_table; counts and profiles are in the order of those 20 letters.
 * The COUNTS are the exact part: a file or a keep / drop decision should take d_counts through gmg_entropy_from_counts, which is
 * the reference's arithmetic on the host bit for bit.  d_dist is finished on the device in the same order of operations and differs
 * only through the device's log and d * d in place of pow (d, 2): below 1e-13 on both distances, NaN where the host gives NaN (a
 * region of one amino acid), ratio = the IEEE quotient of the two distances (1.0 for 0 / 0, 1e3 for x / 0). */
typedef struct gmg_gene_region { uint32_t read; int32_t first, len, strand; } gmg_gene_region;
/* regions: HOST array.  d_counts [n][20] int32 and d_dist [n][3] double {pos_dist, neg_dist, ratio}: DEVICE, either may be NULL.
 * first in [0, read length), 0 <= len <= read length, strand != 0: GMG_ERANGE otherwise; an aa entry that is neither 'A'..'Z' nor
 * '*': GMG_EINVAL.  Stream-ordered: the call waits once for `stream` (the read lengths come back over it for the checks), then
 * queues its kernel and returns; its scratch goes back to the library's cache behind that kernel. */
int gmg_entropy_regions(const gmg_reads *reads, const gmg_gene_region *regions, uint64_t n, const char aa[64],
                        const double pos[20], const double neg[20], int32_t *d_counts, double *d_dist, void *stream);
/* the same for every ORF of a gmg_find_orfs / gmg_mg_score_reads result, which stays on the device: ORF k's region by
 * Entropy_Filter's rule (long-orfs.cc:370-377) from its stop_position, gene_len and frame -- 1-based start stop_position - gene_len
 * (forward) or stop_position + gene_len + 2 (reverse), brought onto the sequence as On_Seq_1 does (long-orfs.cc:1051-1065), len =
 * gene_len -- modulo the read's length.  Rows in the result's ORF order. */
int gmg_entropy_orfs(const gmg_reads *reads, const gmg_mg_result *orfs, const char aa[64], const double pos[20],
                     const double neg[20], int32_t *d_counts, double *d_dist, void *stream);
/* host, libm, the reference's order of operations: the bit-identical finish of one count vector (any output may be NULL) */
int gmg_entropy_from_counts(const int32_t counts[20], const double pos[20], const double neg[20],
                            double *pos_dist, double *neg_dist, double *ratio);
/* DEFAULT_POS_ENTROPY_PROF / DEFAULT_NEG_ENTROPY_PROF (src/Common/gene.hh:47-52) */
int gmg_entropy_default_profiles(double pos[20], double neg[20]);

/* ---- gene coordinates audited: anomaly and start-codon-distrib without the text ------------------------
 * What src/Glimmer/anomaly.cc:76-240 and src/Util/start-codon-distrib.cc:84-106 look at in every gene of a coordinate list, for a
 * batch of regions in one call.  A region is a gmg_gene_region with the meaning gmg_entropy_regions gives it: `len` bases of read
 * `read` from the 0-based `first`, upwards (strand > 0) or downwards and complemented (strand < 0), positions modulo THAT read's
 * length; offsets below count bases of the region in its reading direction.  A codon is named by 16*b0 + 4*b1 + b2 (a=0 c=1 g=2
 * t=3) of its three bases in reading direction.
 * The reference compares raw lower-cased letters with strncmp (anomaly.cc:254-286), no IUPAC matching: amb_base[0 .. n_amb) are the
 * ascending job-wide indices of the bases whose letter is outside acgtACGT (gmg_fasta_ambiguous's indices; NULL with n_amb = 0), and
 * a codon that holds one matches no pattern and has the code -1.
 * Every output is an integer: there is no tolerance. */
typedef struct gmg_audit_params {
    int32_t n_start_codons, n_stop_codons;          /* 0 .. 8 each */
    char start_codon[8][4], stop_codon[8][4];       /* three lower-case letters of a c g t and a NUL; anything else: GMG_EINVAL */
    int32_t flags;                                  /* GMG_AUDIT_NEXT_STOP */
    int32_t reserved;
} gmg_audit_params;
#define GMG_AUDIT_NEXT_STOP 1   /* fill next_stop for the regions whose last codon is no stop codon */
typedef struct gmg_gene_audit {
    int32_t first_codon, last_codon;  /* the region's first / last three bases; -1: len < 3, or one of them is in amb_base */
    int32_t start_which, stop_which;  /* index in start_codon of the first codon / in stop_codon of the last codon (the first of equal
                                         patterns); -1 none */
    int32_t n_inner_stops;            /* stop codons at offsets i = 0, 3, 6, ... with i < len - 3 (anomaly.cc:190-192, 224-231) */
    uint32_t inner_begin;             /* their offsets: inner[inner_begin .. inner_begin + n_inner_stops), ascending */
    int32_t last_back_stop;           /* the largest i of len - 6, len - 9, ..., i >= 0, whose codon is a stop; -1 none (anomaly.cc:209-211) */
    int32_t next_stop;                /* the smallest j of len, len + 3, ..., j < read length, whose codon (offsets j .. j + 2, modulo the
                                         read) is a stop; -1: none, or not asked for, or the last codon is a stop (anomaly.cc:157-176) */
} gmg_gene_audit;
typedef struct gmg_audit gmg_audit;
/* regions: HOST array, any order, repeats allowed.  first in [0, read length), 0 <= len <= read length, strand != 0, read < n_reads,
 * a read of fewer than 2^31 bases: GMG_ERANGE naming the first bad region otherwise, and nothing is returned.  n = 0 gives a valid
 * empty result.  More inner stops in total than mg_max_entries (gmg_set_option): GMG_ETOOBIG, never a truncated list.
 * Stream-ordered; the call itself waits once for the count pass (the size of the list).  The result lives on the device until
 * gmg_audit_fetch, which synchronises the stream the call ran on; free the handle before that stream is destroyed. */
int gmg_genes_audit(const gmg_reads *reads, const struct gmg_gene_region *regions, uint64_t n, const gmg_audit_params *params,
                    const uint64_t *amb_base, uint64_t n_amb, gmg_audit **out, void *stream);
int gmg_audit_info(const gmg_audit *a, uint64_t *n_regions, uint64_t *n_inner);
/* HOST arrays, any may be NULL: records[n_regions], inner[n_inner], first_codon_hist[c] = the number of regions with first_codon ==
 * c, bin 64 those with -1 (counted on the device in the same call). */
int gmg_audit_fetch(const gmg_audit *a, gmg_gene_audit *records, int32_t *inner, int64_t first_codon_hist[65]);
int gmg_audit_free(gmg_audit *a);

/* ---- window composition and uncovered regions: window-acgt and uncovered without the text ----------------
 * gmg_window_counts: what src/Util/window-acgt.cc:63-137 counts (Subscript, :233-252) for every window of every read of a batch.
 * A read of L bases has, with W = window_len and S = window_skip (the reference's ring buffer worked out):
 *   L = 0               no window
 *   0 < L < W           one window, the whole read
 *   L >= W              the full windows at the 0-based offsets 0, S, .. , k S with k = (L - W) / S, and, when (L - W) % S != 0
 *                       and (k + 1) S < L, ONE more from (k + 1) S to the read's end; nothing after it
 * Window j of read r is row read_window_off[r] + j; it starts at offset j S and is min (W, L - j S) bases long, which is why neither
 * is stored.  A row is {a, c, g, t, other}: `other` = the bases of the window that are in amb_base[0 .. n_amb), the ascending
 * job-wide indices of the bases whose letter is outside acgtACGT (gmg_fasta_ambiguous's indices; NULL with n_amb = 0); the four
 * letter counts cover the rest (the code the packed batch holds at a listed base is taken off again).
 * window_len < 1 or window_skip < 1: GMG_EINVAL; a list that does not ascend strictly or reaches total_bases: GMG_EINVAL; a read
 * of 2^31 bases or more: GMG_ERANGE; more windows than mg_max_entries (gmg_set_option): GMG_ETOOBIG, never a truncated table.
 * reads: a device batch; amb_base: HOST.  Stream-ordered; the call itself waits once for the number of windows.  The result lives
 * on the device until gmg_windows_fetch, which synchronises the stream the call ran on; free the handle before that stream is
 * destroyed.  Every output is an integer: there is no tolerance. */
typedef struct gmg_windows gmg_windows;
int gmg_window_counts(const gmg_reads *reads, int64_t window_len, int64_t window_skip, const uint64_t *amb_base, uint64_t n_amb,
                      gmg_windows **out, void *stream);
int gmg_windows_info(const gmg_windows *w, uint64_t *n_reads, uint64_t *n_windows);
/* HOST arrays, either may be NULL: read_window_off[n_reads + 1], counts[n_windows][5] */
int gmg_windows_fetch(const gmg_windows *w, uint64_t *read_window_off, int32_t *counts);
/* the same two arrays where they are: DEVICE pointers, valid until gmg_windows_free, written in the order of the call's stream */
int gmg_windows_device(const gmg_windows *w, const uint64_t **d_read_window_off, const int32_t **d_counts);
int gmg_windows_free(gmg_windows *w);

/* gmg_regions_uncovered: Coalesce_Regions + Output_Uncovered (src/Util/uncovered.cc:186-288): the stretches of every read that none
 * of the intervals covers.  Per read the intervals are taken in ascending lo with the running maximum of hi: a gap [a, b) lies in
 * front of every interval whose lo exceeds the maximum so far (a = that maximum, 0 at the read's start, b = lo), one more runs from
 * the final maximum to the read's end.  A gap is kept when len > 0 && len >= min_len.  A read without intervals gives the gap
 * [0, L), an empty read none; touching intervals merge; an empty interval inside a gap splits it.
 * Gaps come out as gmg_gene_region {read, first = a, len = b - a, strand = +1}, by read and then ascending: gaps[read_gap_off[r] ..
 * read_gap_off[r + 1]) are read r's.
 * intervals: HOST array, any order.  0 <= lo <= hi <= read length and read < n_reads, every read shorter than 2^31 bases:
 * GMG_ERANGE naming the first bad interval otherwise, and nothing is returned.  n = 0 is valid.  More gaps than mg_max_entries:
 * GMG_ETOOBIG.  Stream-ordered; the call itself waits once for the number of gaps; gmg_gaps_fetch synchronises that stream. */
typedef struct gmg_interval { uint32_t read; int32_t lo, hi; } gmg_interval;   /* 0-based, half open: bases lo .. hi - 1 of read `read` */
typedef struct gmg_gaps gmg_gaps;
int gmg_regions_uncovered(const gmg_reads *reads, const gmg_interval *intervals, uint64_t n, int64_t min_len, gmg_gaps **out,
                          void *stream);
int gmg_gaps_info(const gmg_gaps *g, uint64_t *n_gaps);
/* HOST arrays, either may be NULL: gaps[n_gaps], read_gap_off[n_reads + 1] */
int gmg_gaps_fetch(const gmg_gaps *g, struct gmg_gene_region *gaps, uint64_t *read_gap_off);
int gmg_gaps_free(gmg_gaps *g);
/* host only.  Coordinate lines to intervals: the arithmetic of uncovered (src/Util/uncovered.cc:87-174) on gmg_coord lines under the
 * GMG_COORD_USE_DIR / NOWRAP / SKIP_START / SKIP_STOP flags of gmg_extract_plan.  Unlike that planner there is no length test, a
 * region that runs over the sequence's end (the start, on the reverse strand) becomes TWO intervals, and the reverse strand's i =
 * start, j = i - extract_len give [j, i).  intervals: room for 2 n entries; *n_intervals of them are written, in the order of the
 * lines.  GMG_ERANGE naming the line: a read index beyond n_reads, a read of 2^31 bases or more, and every line at which the
 * reference's own arithmetic leaves 0 <= lo <= hi <= L (it prints from outside its string there). */
int gmg_uncovered_plan(const uint64_t *base_offsets, uint64_t n_reads, const gmg_coord *coords, uint64_t n, int flags,
                       gmg_interval *intervals, uint64_t *n_intervals);

/* ---- build-icm: training counts on the device ---------------------------------------
 * Replaces the counting of ICM_Training_t: Count_Char_Pairs for the roots (src/ICM/icm.cc:1841-1870, called from
 * Train_Model, icm.cc:1373-1390), Count_Char_Pairs_Restricted + Get_Training_Node for every deeper level
 * (icm.cc:1190-1256, called from Complete_Tree, icm.cc:1082-1083) and Count_Single_Chars (icm.cc:1874-1896).
 * `strings` = the training strings as a gmg_reads batch, in the orientation Train_Model gets them (build-icm -r
 * reverses them first); it must outlive the trainer.  The tree is built level by level, as in the reference: */
typedef struct gmg_trainer gmg_trainer;
int gmg_trainer_create(const gmg_reads *strings, int model_len, int model_depth, int periodicity, gmg_trainer **out);
/* The 4 x 4 pair tables of tree level `level` (0 = the roots).  Levels are taken in order 0, 1, .. model_depth.
 * For level >= 1, mip_prev[f * 4^(level-1) + k] = mut_info_pos the caller chose for node k of level - 1 in sub-model f
 * (< 0: the tree stops there, its windows count no further).  counts (HOST, periodicity * 4^level * npos * 16 int32,
 * npos = max(model_len - 1, 1)):  counts[((f * 4^level + k) * npos + i) * 16 + 4 * code(w[i]) + code(w[model_len-1])]
 * = number of complete windows w of sub-model f that reach node k of the level -- the reference's
 * train[f][first + k].count[i][pair] (src/ICM/icm.hh:88-101).  A window starting at offset s of its string belongs to
 * sub-model (model_len + s) mod periodicity (icm.cc:1203-1226).  With model_len = 1 only entry [last] of table 0 counts. */
int gmg_trainer_level_counts(gmg_trainer *t, int level, const int16_t *mip_prev, int32_t *counts);
int gmg_trainer_free(gmg_trainer *t);

/* ---- Phymm's classification step: every read against a database of ICMs -------------------------------
 * Glimmer-MG's pipeline classifies reads with Phymm first: scoreReadsGlim.pl scores every read and its reverse complement
 * under every ICM of a database (simple-score, the values printed with %.4f) and writes the raw matrix -- per read the
 * reverse strand's text only when it parses to a strictly greater number; glimmer-mg.py's parse_phymm then keeps the best
 * top_hits informative models of every read with its score_insert.  A gmg_tophits handle keeps those slots in HBM while the
 * database streams through in batches of B models ([B][n_reads][2] sums, as gmg_score_reads_strings writes them).
 * Scores are compared as the printed text orders them: the key of a value is its %.4f digits as an integer count of 1e-4
 * units (glibc's rounding: the exact binary value, ties to even).  A value that is not finite or whose magnitude is
 * 2^52 / 10^4 or more has no key here: GMG_ERANGE (after which the slots are undefined). */
#define GMG_TOPHITS_MAX 16
/* the most bytes one field of gmg_tophits_format_rows takes: sign, 12 integer digits, '.', 4 decimals, separator */
#define GMG_TOPHITS_MAX_FIELD 19
typedef struct gmg_tophits gmg_tophits;
/* empty slots for every read of `reads` (which must outlive the handle); top_hits 1 .. GMG_TOPHITS_MAX */
int gmg_tophits_create(const gmg_reads *reads, int top_hits, gmg_tophits **out);
int gmg_tophits_free(gmg_tophits *h);
/* score_insert of models first_model .. first_model + B - 1 (in that order) for every read: d_sums (device) [B][n_reads][2];
 * informative (HOST, B entries; NULL = all) skips the models whose entry is 0; forward_only != 0 takes [..][0] alone (the
 * script's -f).  The first top_hits models fill the empty slots in arrival order, unsorted; a later one goes in at the first
 * slot it strictly beats, the slots behind move down.  Synchronises `stream`. */
int gmg_tophits_update_sums(gmg_tophits *h, const double *d_sums, int B, int first_model, const uint8_t *informative,
                            int forward_only, void *stream);
/* gmg_score_reads_strings of the B models into a scratch buffer the handle owns (and reuses), then gmg_tophits_update_sums;
 * *d_sums_out (may be NULL) = that buffer, valid until the next call on the handle */
int gmg_tophits_scores(gmg_tophits *h, const gmg_model *const *models, int B, int first_model, const uint8_t *informative,
                       int forward_only, void *stream, const double **d_sums_out);
/* the slots (HOST, [n_reads][top_hits]): keys (the %.4f value x 10^4) and model indices; an empty slot has model -1.  Copied on the
 * stream of the handle's last update (the default stream before the first), which must still exist, and waited for. */
int gmg_tophits_fetch(const gmg_tophits *h, int64_t *keys, int32_t *models);
/* The B data-matrix lines of the raw file for d_sums (device, [B][n_reads][2]): per model one line, per read the winning
 * strand's %.4f text, tab-separated, ending in a newline -- formatted on the device.  *bytes: in = capacity of host_out, out =
 * the length of the lines; host_out NULL only asks for that length, a smaller capacity is GMG_ERANGE.  B * n_reads *
 * GMG_TOPHITS_MAX_FIELD bytes (B without reads) always suffice.  Synchronises `stream`. */
int gmg_tophits_format_rows(gmg_tophits *h, const double *d_sums, int B, int forward_only, char *host_out, size_t *bytes,
                            void *stream);

/* ---- feature models from predictions: scripts/train_features.py --predict P --seq S -----------------------
 * After a run of the pipeline the reference retrains what the next run reads with -f: the length distributions of genes and of
 * non-gene ORFs, the start-codon counts and the adjacent-orientation / adjacent-distance distributions (parse_genes,
 * train_features.py:223-280; forward_parse_nongenes, :320-467, on every sequence and on its reverse complement;
 * destrand_orientations, :544-554).  The non-gene side walks back from every stop codon of all six frames: that runs here.
 * A gene is one line of the predict file as parse_predict (:163-199) leaves it: `read` in the batch, the sign of its frame
 * field, the 0-based half-open [start, end) CLIPPED to the read (0 <= start, end <= length: GMG_ERANGE otherwise) and whether the
 * end that holds its start codon lies inside the read.  The genes of a read are consecutive and keep the file's order; reads
 * come in the order of their first gene line (the reference iterates a Python 2 dict: unspecified there); a read without genes
 * takes no part at all.  opaque_base[0 .. n_opaque): the ascending job-wide indices of the bases whose letter is not an upper-case
 * A C G T (gmg_fasta_not_upper_acgt): a codon with such a base is neither a start nor a stop on either strand.
 * Integer counts are exact; every fractional bin is the sequential IEEE double sum of its 1.0 / num_starts terms in the reference's
 * order (pass +1 before pass -1, reads in order, stops ascending with L, L + 1, L + 2 last, starts descending, the preceding gene
 * before the succeeding one), bit for bit.
 * GMG_ETOOBIG, never a truncated result: a read whose positions do not fit int32, more orientation / distance records than
 * mg_max_entries (gmg_set_option).  Synchronises `stream`; the result lives on the host. */
typedef struct gmg_feature_gene { uint32_t read; int32_t strand, start, end, start_codon; } gmg_feature_gene;
typedef struct gmg_features_params {
    int32_t min_length;          /* -l, default 75: shorter ORFs count in the length histogram only */
    int32_t max_overlap;         /* -o, default 50; 0 .. 2^20                                       */
    int32_t drop_tga;            /* -z: TGA is no stop codon                                        */
    int32_t reserved;
} gmg_features_params;
/* One table (GENE or NON) after destrand_orientations.  lengths[l], l < n_lengths = 1 + the largest bin (0: none); starts in the
 * order ATG GTG TTG; orient in the order (1,1) (1,-1) (-1,1) (-1,-1), orient_raw the four sums before destranding;
 * dist[k][j], j < n_dist[k]: the bin of distance j - max_overlap under orientation k = (1,1) (1,-1) (-1,1), up to the largest
 * bin present (n_dist[k] = 0: the table is empty).  The arrays belong to the handle (or, for gmg_features_format, the caller). */
typedef struct gmg_features_table {
    uint64_t n_lengths;
    const int64_t *lengths;
    int64_t starts[3];
    double orient[4], orient_raw[4];
    uint64_t n_dist[3];
    const double *dist[3];
} gmg_features_table;
typedef struct gmg_features gmg_features;
int gmg_features_count(const gmg_reads *reads, const gmg_feature_gene *genes, uint64_t n_genes, const uint64_t *opaque_base,
                       uint64_t n_opaque, const gmg_features_params *params, gmg_features **out, void *stream);
#define GMG_FEATURES_GENE 0
#define GMG_FEATURES_NON 1
int gmg_features_fetch(const gmg_features *f, int which, gmg_features_table *out);
/* units of 32 positions the item kernels ran, orientation / distance records, and the time of the call's stages in ms (any pointer
 * may be NULL).  Between events on the stream: [0] opaque bits + codon classes (with the uploads), [1] count pass, [2] scan, [3] write
 * pass, [4] sorts + in-order sums.  On the host's clock: [5] the extents of the reads that have genes read back + the gene list, [6] from the first to the
 * last of those events, [7] the histograms read back + destranding. */
#define GMG_FEATURES_STAGES 8
int gmg_features_info(const gmg_features *f, uint64_t *n_units, uint64_t *n_records, float *stage_ms);
int gmg_features_free(gmg_features *f);
/* host only.  The ascending job-wide indices (as gmg_fasta_ingest numbers the bases) of the sequence bytes of `bytes` that are not
 * one of A C G T; counts and sizes as gmg_fasta_ambiguous does. */
int gmg_fasta_not_upper_acgt(const char *bytes, uint64_t n_bytes, uint64_t *base, uint64_t cap, uint64_t *n);
/* host only.  The text the script writes for one table: what = GMG_FEATURES_BLOCK the table's six sections of the feature file
 * (output_featurefile, :630-673, titles with orf_type "GENE" / "NON"), or the body of one of output_stats' files (:562-623):
 * _LENGTHS, _STARTS, _ORIENTS, _DIST + k.  Formats %d and %.1f, ranges from 0 (lengths) and -max_overlap (distances) to the largest
 * bin, as there; an empty table prints no line (under -f the reference dies on an empty length table).
 * *bytes: in = room at out, out = the length of the text (no terminator); out NULL only asks for the length, a smaller room is
 * GMG_ERANGE. */
#define GMG_FEATURES_BLOCK 0
#define GMG_FEATURES_LENGTHS 1
#define GMG_FEATURES_STARTS 2
#define GMG_FEATURES_ORIENTS 3
#define GMG_FEATURES_DIST 4
int gmg_features_format(const gmg_features_table *t, const char *orf_type, int what, int max_overlap, char *out, size_t *bytes);

/* ---- device memory helpers (for callers without their own allocator) -------- */
int gmg_device_malloc(void **d_ptr, size_t bytes);
int gmg_device_free(void *d_ptr);
int gmg_memcpy_h2d(void *d_dst, const void *src, size_t bytes, void *stream);
int gmg_memcpy_d2h(void *dst, const void *d_src, size_t bytes, void *stream);
/* Page-lock / release a host buffer the caller owns (file bytes, result arrays), so that the copies the library
 * makes from / to it run at PCIe speed. */
int gmg_host_register(void *ptr, size_t bytes);
int gmg_host_unregister(void *ptr);
/* Non-blocking streams for callers without a HIP binding of their own (every `void *stream` parameter takes one). */
int gmg_stream_create(void **stream);
int gmg_stream_destroy(void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GMG_H */
