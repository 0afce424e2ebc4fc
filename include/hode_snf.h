/* C ABI of libhode_snf.so: the Sylvester-flow posterior (LHM-SNF) with its Monte-Carlo KL against the Exponential(100)
 * prior, forward and backward, one launch each, gfx950.  The flows are those of hode_sylvester.h with M == D; here the
 * kernels take the encoder's raw heads and form r1, r2 and Q on chip (they never exist in device memory).
 *
 * Per patient b, flow k and draw s (eps = noise[s][b][:]), with U the strictly-upper mask:
 *     r1 = U * full_d[b][k]   + diag(tanh(diag1[b][k]))
 *     r2 = U * full_d[b][k]^T + diag(tanh(diag2[b][k]))
 *     triangular (n_householder == 0):  p = identity for even k, the flip D-1 .. 0 for odd k (an involution);
 *                                       A[d][m] = r2[m][p[d]],  C[d][m] = r1[p[d]][m]
 *     householder (n_householder = H):  vh = v[b][k][h] / |v[b][k][h]|_2,  Q = (I - 2 v0 v0^T) ... (I - 2 v_{H-1} v_{H-1}^T),
 *                                       A = Q r2^T,  C = Q r1
 *     z0 = eps * exp(0.5 log_var) + mu
 *     a = z A + bias[b][k];  h = tanh(a);  z' = z + h C^T;  logdet += sum_m log|1 + (1 - h[m]^2) r1[m][m] r2[m][m]|
 *     z_out = exp(z_K - 5);  logdet += sum_d (z_K - 5)
 *     kl_s  = sum_d log N(z0; mu, exp(0.5 log_var)) - logdet - sum_d (log 100 - 100 z_out)
 *     kl[b] = mean over s in [s_kl, S) of kl_s
 * (the last four lines are those of hode_flow.h).
 *
 * Conventions as in hode_sylvester.h: row-major float32 device pointers, return 0 on success, <0 an argument error
 * (HODE_SNF_E_*), >0 a hipError_t from the launch; the message is in hode_snf_last_error_string().  An argument error
 * launches nothing: the outputs stay untouched.  The library never allocates: the states z_0 .. z_K of every draw (the
 * tape) and the backward's running cotangent live in a workspace the caller owns, hode_snf_workspace_bytes() large; the
 * forward writes the tape, the backward reads it and writes only the cotangent part.  Domain: latent_dim 1 ..
 * HODE_SNF_MAX_LATENT, n_flows 1 .. HODE_SNF_MAX_FLOWS, n_samples 1 .. HODE_SNF_MAX_SAMPLES, n_householder 0 ..
 * HODE_SNF_MAX_HOUSEHOLDER, batch >= 1, 0 <= s_kl < n_samples.  Sums over draws run in a fixed order on chip (no float
 * atomics): repeated calls are bit-identical. */
#ifndef HODE_SNF_H_
#define HODE_SNF_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HODE_SNF_ABI_VERSION 1
#define HODE_SNF_MAX_LATENT 32
#define HODE_SNF_MAX_FLOWS 16
#define HODE_SNF_MAX_SAMPLES 256
#define HODE_SNF_MAX_HOUSEHOLDER 8

#define HODE_SNF_E_NULL -1      /* a required pointer is NULL */
#define HODE_SNF_E_SIZE -2      /* struct_size mismatch / dimension outside the domain */
#define HODE_SNF_E_WORKSPACE -3 /* workspace missing, too small or not 16-byte aligned */

typedef struct hode_snf_desc {
  uint32_t struct_size;
  int32_t batch;            /* B */
  int32_t latent_dim;       /* D */
  int32_t n_flows;          /* K */
  int32_t n_samples;        /* S */
  int32_t s_kl;             /* first draw of the KL mean, 0 <= s_kl < S (1: draw 0 is the decoder's) */
  int32_t n_householder;    /* H; 0 selects the triangular type */
  const float* mu;          /* [B][D] */
  const float* log_var;     /* [B][D] */
  const float* full_d;      /* [B][K][D][D] */
  const float* diag1;       /* [B][K][D] */
  const float* diag2;       /* [B][K][D] */
  const float* bias;        /* [B][K][D] */
  const float* v;           /* [B][K][H][D]; required when H > 0, ignored otherwise */
  const float* noise;       /* [S][B][D] standard-normal draws */
  float* z_out;             /* forward out [S][B][D], or NULL */
  float* kl;                /* forward out [B] */
  void* workspace;          /* forward out / backward in and out; hode_snf_workspace_bytes() large, 16-byte aligned */
  size_t workspace_bytes;
  const float* grad_z_out;  /* backward in [S][B][D], or NULL (zero) */
  const float* grad_kl;     /* backward in [B], or NULL (zero) */
  float* grad_mu;           /* backward out [B][D] (overwritten) */
  float* grad_log_var;      /* backward out [B][D] */
  float* grad_full_d;       /* backward out [B][K][D][D] (its diagonal is zero) */
  float* grad_diag1;        /* backward out [B][K][D] */
  float* grad_diag2;        /* backward out [B][K][D] */
  float* grad_bias;         /* backward out [B][K][D] */
  float* grad_v;            /* backward out [B][K][H][D]; required when H > 0, ignored otherwise */
} hode_snf_desc;

int hode_snf_version(void);
const char* hode_snf_last_error_string(void);
/* bytes of the workspace for the descriptor's batch, latent_dim, n_flows and n_samples; 0 outside the domain */
size_t hode_snf_workspace_bytes(const hode_snf_desc* desc);
/* kl and (optionally) z_out; writes the tape */
int hode_snf_fwd(const hode_snf_desc* desc, void* hip_stream);
/* reads the forward's tape; every grad_* output of the type is required */
int hode_snf_bwd(const hode_snf_desc* desc, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* HODE_SNF_H_ */
