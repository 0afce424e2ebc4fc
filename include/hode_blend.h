/* C ABI of libhode_blend.so: the scoring arithmetic of the reference's real-data two-model scripts
 * (experiments/run_real_ensemble.py, run_real_residual.py, and the tail of run_real.py), gfx950.
 *
 * hode_blend_nnls2: per forecast step i the non-negative least squares fit of run_real_ensemble.py:109-117,
 *     min_{w >= 0} sum_r (w[0] x_e[i][r] + w[1] x_m[i][r] - truth[i][r])^2     over the `rows` = B * obs entries of the step
 * (the fit does not read the mask, as in the reference).  The five Gram sums a11 = sum x_e^2, a22 = sum x_m^2,
 * a12 = sum x_e x_m, b1 = sum x_e truth, b2 = sum x_m truth are reduced in float64 (fp32 x fp32 products are exact there) and
 * the problem is solved in float64 in closed form: with det = a11 a22 - a12^2 > 0 and both unconstrained weights > 0 the
 * unconstrained solution; otherwise the better of (max(b1 / a11, 0), 0) and (0, max(b2 / a22, 0)) by residual decrease
 * b_i^2 / a_ii over positive b_i (a column with a_ii = 0 gets weight 0; on an exact tie the first column wins).  An
 * inactive weight is exactly 0.0.  When det <= 0 (one row, collinear columns) the minimiser is not unique: the result is
 * a finite, non-negative minimiser of the objective.  The solve is plain IEEE float64 without contraction, and the
 * unconstrained candidate is taken only if its own residual decrease 2 u.b - u'Gu reaches that of the better single
 * column (less 1e-9 of it), which the true minimiser always does: collinear columns whose rounded determinant comes out
 * a positive residue of rounding do not end in weights that are noise over noise.
 *
 * hode_blend_horizon_sse: per patient p and horizon h, over the forecast steps t < horizons[h] and the components o,
 *     sse[h][p] = sum (truth - (w_e[t][o] x_e + w_m[t][o] x_m))^2 mask        cnt[h][p] = sum mask
 * with x_m NULL for a single model and each weight table NULL for one.  Every input is read once; the horizons are
 * prefixes of one running sum.  Terms are formed in float32 and accumulated in float64; outputs are float32.
 *
 * Conventions as in hode_mix.h: row-major float32 device pointers, element strides, return 0 on success, <0 an argument
 * error (HODE_BLEND_E_*, nothing is launched), >0 a hipError_t from the launch; the message is in
 * hode_blend_last_error_string().  The library allocates nothing.  Every sum runs in a fixed order (no float atomics):
 * repeated calls are bit-identical.
 * Domain: every dimension >= 1; obs_dim in 1 .. HODE_BLEND_MAX_OBS; n_horizons in 1 .. HODE_BLEND_MAX_HORIZONS with
 * 1 <= horizons[0] <= horizons[1] <= ... (each is clipped to n_times); rows and n_times * batch below 2^31. */
#ifndef HODE_BLEND_H_
#define HODE_BLEND_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HODE_BLEND_ABI_VERSION 1
#define HODE_BLEND_MAX_OBS 128
#define HODE_BLEND_MAX_HORIZONS 8

#define HODE_BLEND_E_NULL -1        /* a required pointer is NULL */
#define HODE_BLEND_E_SIZE -2        /* struct_size mismatch / dimension, stride or horizon outside the domain */

typedef struct hode_blend_nnls2_desc {
  uint32_t struct_size;
  int32_t n_steps;          /* T' */
  int64_t rows;             /* B * obs entries per step, contiguous */
  int64_t step_stride_e;    /* element strides between steps; rows for a contiguous (T', B, obs) tensor */
  int64_t step_stride_m;
  int64_t step_stride_b;
  const float* x_e;         /* first column: the expert's forecast */
  const float* x_m;         /* second column */
  const float* truth;       /* right-hand side */
  float* w;                 /* out [T'][2] */
} hode_blend_nnls2_desc;

typedef struct hode_blend_horizon_desc {
  uint32_t struct_size;
  int32_t n_times;          /* T' */
  int32_t batch;            /* B */
  int32_t obs_dim;          /* obs */
  int32_t n_horizons;       /* H */
  int32_t reserved;         /* 0 */
  int32_t horizons[HODE_BLEND_MAX_HORIZONS]; /* horizon ends in forecast steps, non-decreasing, the first H are read */
  /* element strides of x_e, x_m, truth and mask along time and patient (the component axis is contiguous): B * obs, obs */
  int64_t time_stride;
  int64_t patient_stride;
  const float* x_e;         /* [T'][B][obs] */
  const float* x_m;         /* [T'][B][obs], or NULL (single model) */
  const float* w_e;         /* [T'][obs] mixing weights of x_e, or NULL (one) */
  const float* w_m;         /* [T'][obs] mixing weights of x_m, or NULL (one) */
  const float* truth;       /* [T'][B][obs] */
  const float* mask;        /* [T'][B][obs] */
  float* sse;               /* out [H][B] */
  float* cnt;               /* out [H][B] */
} hode_blend_horizon_desc;

int hode_blend_version(void);
const char* hode_blend_last_error_string(void);
int hode_blend_nnls2(const hode_blend_nnls2_desc* desc, void* hip_stream);
int hode_blend_horizon_sse(const hode_blend_horizon_desc* desc, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* HODE_BLEND_H_ */
