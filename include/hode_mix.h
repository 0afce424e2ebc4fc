/* C ABI of libhode_mix.so: the ensemble CRPS of a weighted sum of TWO models' posterior forecasts, the metric of the
 * reference's training_utils.evaluate_ensemble / evaluate_ensemble_horizon (training_utils.py:383-565), one launch, gfx950.
 *
 * Per forecast row (t, b), observed component o and ensemble member m = 0 .. M-1:
 *     v_m        = mix_e[t][o] * (w_e[o][:] . h_e[t][m][b][:] + b_e[o])  +  mix_m[t][o] * (w_m[o][:] . h_m[t][m][b][:] + b_m[o])
 *     crps[t][b][o] = 1/M sum_m |v_m - truth[t][b][o]|  -  1/M^2 sum_{i<j} |v_i - v_j|     (properscoring, equal weights)
 *     crps_sum[t][b] = sum_o crps[t][b][o]
 * Neither model's readout is materialised.  The two latent widths are independent.
 *
 * Conventions as in hode.h: row-major float32 device pointers, return 0 on success, <0 an argument error
 * (HODE_MIX_E_*), >0 a hipError_t from the launch; the message is in hode_mix_last_error_string().  Every sum runs in a
 * fixed order on chip (no float atomics): repeated calls are bit-identical.
 * Domain: obs_dim, n_members, latent_dim_e, latent_dim_m in 1 .. HODE_MIX_MAX_DIM, n_times * batch < 2^31, and the
 * workgroup's LDS (see hode_mix.hip: mix_lds_bytes plus the kernel's static block) at most 160 KiB. */
#ifndef HODE_MIX_H_
#define HODE_MIX_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HODE_MIX_ABI_VERSION 1
#define HODE_MIX_MAX_DIM 128

#define HODE_MIX_E_NULL -1        /* a required pointer is NULL */
#define HODE_MIX_E_SIZE -2        /* struct_size mismatch / dimension or stride outside the domain */
#define HODE_MIX_E_UNSUPPORTED -3 /* the shape needs more LDS than a workgroup has */

typedef struct hode_mix_crps_desc {
  uint32_t struct_size;
  int32_t n_times;          /* T' */
  int32_t batch;            /* B */
  int32_t n_members;        /* M */
  int32_t obs_dim;          /* obs */
  int32_t latent_dim_e;     /* De */
  int32_t latent_dim_m;     /* Dm */
  int32_t reserved;         /* 0 */
  /* element strides of h_e / h_m along time, member and patient (the latent axis is contiguous); for a decoder output
   * (T', M * B, D) with a member-major batch axis: M * B * D, B * D, D */
  int64_t time_stride_e, member_stride_e, patient_stride_e;
  int64_t time_stride_m, member_stride_m, patient_stride_m;
  const float* h_e;         /* latent trajectories of the first model */
  const float* h_m;         /* latent trajectories of the second model */
  const float* w_e;         /* [obs][De] readout of the first model */
  const float* b_e;         /* [obs], or NULL (zero) */
  const float* w_m;         /* [obs][Dm] readout of the second model */
  const float* b_m;         /* [obs], or NULL (zero) */
  const float* mix_e;       /* [T'][obs] mixing weights of the first model, or NULL (one) */
  const float* mix_m;       /* [T'][obs] mixing weights of the second model, or NULL (one) */
  const float* truth;       /* [T'][B][obs] */
  float* crps;              /* out [T'][B][obs], or NULL */
  float* crps_sum;          /* out [T'][B], or NULL; at least one of the two outputs */
} hode_mix_crps_desc;

int hode_mix_version(void);
const char* hode_mix_last_error_string(void);
int hode_mix_crps(const hode_mix_crps_desc* desc, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* HODE_MIX_H_ */
