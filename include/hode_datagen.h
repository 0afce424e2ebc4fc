/* C ABI of libhode_datagen.so: the synthetic data generator of the reference's simulation experiments
 * (dataloader.py DataGeneratorRoche.solve / generate_data), gfx950.
 *
 * hode_datagen_generate integrates, per patient n, the TRUE hybrid ODE from init[n] over the grid t_i = i * step,
 * i = 0 .. n_times - 1, in float64:
 *     Disease'     = Disease k_disprog - Disease Immunity^HillCure k_discure_immunity - Disease ImmuneReact k_discure_immunereact
 *     ImmuneReact' = Disease k_immune_disease - ImmuneReact k_immune_off + Disease ImmuneReact k_immune_feedback
 *                    + ImmuneReact^HillPatho emax / (ec50^HillPatho + ImmuneReact^HillPatho) - Dose2 ImmuneReact k_dexa
 *     Immunity'    = ImmuneReact k_immunity
 *     Dose2'       = kel Dose(t) - kel Dose2,   Dose(t) = dose_amount[n] * sum over doses with tau_k <= t of exp(kel (tau_k - t))
 *     learned'     = tanh(y @ ml_coef)                                              (latent_dim > 4)
 * with a per-patient adaptive Dormand-Prince 5(4) pair (RMS error norm over atol + rtol max(|y|, |y_new|), safety 0.9,
 * growth at most 10, shrink at most 0.2, FSAL inside a smooth piece).  A grid interval is split at every dose time
 * strictly inside it and the set of active doses is fixed per piece, so the right-hand side is smooth within every step.
 *
 * Per grid point i and patient n it writes, time-major and float32 like the reference's tensors:
 *     latents[i][n][:]      = y
 *     actions[i][n][0]      = dose_amount[n] if some dose time equals i * step, else 0
 *     raw[i][n][o]          = float32(output_coef[o][:D] . y + output_coef[o][D] + sigma * eps[i][n][o])
 *     measurements[i][n][o] = float32((raw - mean_o) / std_o),  mean_o and the unbiased std_o over all n_times * n_patients
 *                             raw values of channel o, summed in float64 in a fixed order
 *     masks[i][n][o]        = (u[i][n][o] > p_remove) * (patient n alive at i)
 * eps is noise[i][n][o] when `noise` is given.  Otherwise it comes from Philox4x32-10 with key (seed low word, seed high
 * word) and counter (i, n, o, stream): eps = sqrt(-2 ln u1) cos(2 pi u2) in float64 with u1, u2 = (word 0, word 1 + 0.5) / 2^32
 * of stream 0; u = (word 0 + 0.5) / 2^32 of stream 1.  A value depends on the seed and the element only, never on the
 * launch geometry.  noise_out, when given, receives the eps used, in float64.
 *
 * A patient whose state is not finite, or who needs more than max_steps attempted steps inside one grid interval, stops:
 * status[n] is the first grid index it has no state for (-1 if that is index 0, i.e. init[n] is not finite; 0 = fine), and
 * from that index on its latents, actions and measurements are 0 and its masks 0.  Its missing raw values enter mean and
 * std as the zeros the reference pads with.
 *
 * Conventions as in hode_blend.h: row-major device pointers, return 0 on success, <0 an argument error (HODE_DATAGEN_E_*,
 * nothing is launched), >0 a hipError_t from a launch; the message is in hode_datagen_last_error_string().  The library
 * allocates nothing: the caller hands it hode_datagen_workspace_bytes(n_patients, obs_dim) bytes of 8-byte aligned
 * device memory, whose first 2 * obs_dim doubles hold mean[obs] and std[obs] afterwards.  No float atomics: repeated calls
 * are bit-identical.
 * Domain: latent_dim in {4, 6, 8, 12, 20}; 1 <= obs_dim <= HODE_DATAGEN_MAX_OBS; 1 <= n_dose <= HODE_DATAGEN_MAX_DOSES;
 * n_times >= 2; n_patients >= 1; n_times * n_patients < 2^31; step > 0; rtol, atol >= 0 and not both 0; max_steps >= 1. */
#ifndef HODE_DATAGEN_H_
#define HODE_DATAGEN_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HODE_DATAGEN_ABI_VERSION 1
#define HODE_DATAGEN_MAX_OBS 128
#define HODE_DATAGEN_MAX_DOSES 8
#define HODE_DATAGEN_N_THETA 13

#define HODE_DATAGEN_E_NULL -1         /* a required pointer is NULL */
#define HODE_DATAGEN_E_SIZE -2         /* struct_size mismatch / a size, tolerance or the workspace outside the domain */
#define HODE_DATAGEN_E_UNSUPPORTED -3  /* latent_dim has no compiled kernel / unknown flag */

typedef struct hode_datagen_desc {
  uint32_t struct_size;
  int32_t n_patients;       /* N */
  int32_t n_times;          /* T grid points, t_i = i * step */
  int32_t latent_dim;       /* D */
  int32_t obs_dim;          /* obs */
  int32_t n_dose;           /* K doses per patient */
  int32_t max_steps;        /* attempted steps per grid interval */
  uint32_t flags;           /* 0 */
  uint64_t seed;
  double step;
  double rtol;
  double atol;
  double sigma;             /* output noise scale */
  double p_remove;
  /* HillCure, HillPatho, ec50_patho, emax_patho, k_dexa, k_discure_immunereact, k_discure_immunity, k_disprog,
   * k_immune_disease, k_immune_feedback, k_immune_off, k_immunity, kel: host values */
  double theta[HODE_DATAGEN_N_THETA];
  const double* init;        /* [N][D] */
  const double* dose_times;  /* [N][K] */
  const double* dose_amount; /* [N] */
  const double* ml_coef;     /* [D][D - 4], unused (may be NULL) when D = 4 */
  const double* output_coef; /* [obs][D + 1], the last column is the offset */
  const float* noise;        /* [T][N][obs], or NULL: drawn in the kernel */
  float* latents;            /* out [T][N][D] */
  float* actions;            /* out [T][N][1] */
  float* measurements;       /* out [T][N][obs] */
  float* masks;              /* out [T][N][obs] */
  double* noise_out;         /* out [T][N][obs], or NULL */
  int32_t* status;           /* out [N] */
  int32_t* steps;            /* out [N] attempted steps of the patient over the whole grid, or NULL */
  void* workspace;
  uint64_t workspace_bytes;
} hode_datagen_desc;

int hode_datagen_version(void);
const char* hode_datagen_last_error_string(void);
/* 0 if the sizes are outside the domain */
uint64_t hode_datagen_workspace_bytes(int32_t n_patients, int32_t obs_dim);
int hode_datagen_generate(const hode_datagen_desc* desc, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* HODE_DATAGEN_H_ */
