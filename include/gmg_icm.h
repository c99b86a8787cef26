/*
 * gmg_icm.h -- C ABI over the host-side ICM_t (glimmer-mg_amd/host/icm.hh) for
 * FFI users that cannot include the C++ class.  Model I/O and the null-model
 * builder are host code, as in the reference (src/ICM/icm.cc:65-216, 614-803);
 * nothing here scores (gmg_icm_train counts on the device).  Status codes and gmg_last_error() as in gmg.h; no
 * function exits the process.
 */
#ifndef GMG_ICM_H
#define GMG_ICM_H

#include "gmg.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gmg_icm gmg_icm;   /* owns one ICM_t */

/* ICM_t::ICM_t(m, d, p)                          src/ICM/icm.cc:24-44   */
int gmg_icm_new(int model_len, int model_depth, int periodicity, gmg_icm **out);
/* ICM_t::Read / Input without the exit()         src/ICM/icm.cc:614-726,846-861 */
int gmg_icm_open(const char *path, gmg_icm **out);
/* ICM_t::Build_Indep_WO_Stops; the model must be (3,2,3)  src/ICM/icm.cc:65-216 */
int gmg_icm_build_indep(gmg_icm *icm, double gc_frac, const char *const *stop_codon, int n_stops);
/* ICM_t::Output(fp, binary)                      src/ICM/icm.cc:729-803,961-998 */
int gmg_icm_write(gmg_icm *icm, const char *path);
int gmg_icm_free(gmg_icm *icm);
/* ICM_Training_t(m, d, p) + Train_Model(data)   src/ICM/icm.cc:1010-1042,1356-1455: a model trained on n_strings
 * NUL-terminated lower-case strings (build-icm's Training_Data).  The counting runs on the device (gmg_trainer_*). */
int gmg_icm_train(const char *const *strings, int n_strings, int model_len, int model_depth, int periodicity,
                  gmg_icm **out);
/* the same from training strings that already are a batch on the device (gmg_reads_extract, gmg_reads_upload): string k is
 * read k; nothing is packed or uploaded.  `strings` stays the caller's. */
int gmg_icm_train_reads(const gmg_reads *strings, int model_len, int model_depth, int periodicity, gmg_icm **out);

int gmg_icm_params(const gmg_icm *icm, int *model_len, int *model_depth, int *periodicity, int *num_nodes);
/* copies mip[P*N] and prob4[P*N*4] (the layout gmg_model_upload takes) */
int gmg_icm_tables(const gmg_icm *icm, int16_t *mip, float *prob4);
/* device mirror of the tables: uploaded on first use, owned by the gmg_icm */
int gmg_icm_device_model(const gmg_icm *icm, const gmg_model **out);

/* ---- fixed-length ICMs (src/ICM/icm.hh:216-289) -------------------------------------------------------------------
 * A gmg_fixed_icm owns one Fixed_Length_ICM_t (the scorer) and, when it was trained here, the Fixed_Length_ICM_Training_t
 * that wrote it (for gmg_fixed_icm_write). */
typedef struct gmg_fixed_icm gmg_fixed_icm;
/* Fixed_Length_ICM_t::read without the exit (src/ICM/icm.cc:1502-1559): GMG_EBADMODEL with the reference's message for a bad
 * version, and for what this library refuses: a length outside 1..32, a permutation that is not a bijection of 0..L-1 */
int gmg_fixed_icm_read(const char *path, gmg_fixed_icm **out);
/* build-fixed: Fixed_Length_ICM_Training_t (L, max_depth, special, perm) + Train_Model on n_strings NUL-terminated strings of
 * length L = strlen(strings[0]) (the strings are copied: the caller's are not permuted); perm = NULL for none */
int gmg_fixed_icm_train(const char *const *strings, int n_strings, int max_depth, int special_position, const int *perm,
                        gmg_fixed_icm **out);
/* Fixed_Length_ICM_Training_t::Output: binary != 0 the model file, 0 the -t text; GMG_EINVAL for a model that was read */
int gmg_fixed_icm_write(gmg_fixed_icm *icm, const char *path, int binary);
/* length, max_depth, special position, model type and the permutation (perm: room for 32 ints, or NULL) */
int gmg_fixed_icm_params(const gmg_fixed_icm *icm, int *length, int *max_depth, int *special_position, int *model_type,
                         int *perm);
/* out[k] = Fixed_Length_ICM_t::subrange_score(strings[k], lo, hi) in ONE device call (Score_Windows); GMG_ERANGE with the
 * reference's "too short" message for the first string it would stop at, GMG_EINVAL for a bad range */
int gmg_fixed_icm_score(gmg_fixed_icm *icm, const char *const *strings, int n_strings, int lo, int hi, double *out);
/* the device copy of all sub-models (gmg_fixed_score), owned by the gmg_fixed_icm */
int gmg_fixed_icm_device_model(gmg_fixed_icm *icm, const gmg_fixed_model **out);
int gmg_fixed_icm_free(gmg_fixed_icm *icm);

#ifdef __cplusplus
}
#endif
#endif
