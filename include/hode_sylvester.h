/* C ABI of libhode_sylvester.so: a chain of K Sylvester normalizing flows (reference flow.py:62-138 Sylvester,
 * flow.py:141-219 TriangularSylvester) over S draws per patient, forward and backward, one launch each, gfx950.  The
 * flow parameters are shared by the draws of a patient.
 *
 * Per patient b, draw s and flow k, with r1 = r1[b][k], r2 = r2[b][k] (full M x M, used as given: no mask is applied):
 *     dense mode (q given):          A = q r2^T,  C = q r1                              (D x M)
 *     triangular mode (q NULL, M == D, p = perm[k] or the identity):
 *                                    A[d][m] = sum over {j : p[j] == d} of r2[m][j],  C[i][m] = r1[p[i]][m]
 *         i.e. a = z[p] r2^T + b,  w = tanh(a) r1^T,  z'[i] = z[i] + w[p[i]]: the output is gathered with the SAME index
 *         as the input (a forward gather, not the inverse permutation; the two agree only for involutions).
 *     a = z A + b[b][k];  h = tanh(a);  z' = z + h C^T
 *     log_diag[s][b][k][m] = log|1 + (1 - h[m]^2) r1[m][m] r2[m][m]|;  logdet[s][b] = sum over k, m of log_diag
 *
 * Conventions as in hode_flow.h: row-major float32 device pointers, return 0 on success, <0 an argument error
 * (HODE_SYLVESTER_E_*), >0 a hipError_t from the launch; the message is in hode_sylvester_last_error_string().  An
 * argument error launches nothing: the outputs stay untouched.  The library never allocates: the forward's tape (z_1 ..
 * z_{K-1} of every draw) lives in a workspace the caller owns, hode_sylvester_workspace_bytes() large, and the backward
 * reads it back.  Domain: latent_dim 1 .. HODE_SYLVESTER_MAX_LATENT, n_ortho 1 .. HODE_SYLVESTER_MAX_ORTHO, n_flows
 * 1 .. HODE_SYLVESTER_MAX_FLOWS, n_samples 1 .. HODE_SYLVESTER_MAX_SAMPLES, batch >= 1.  Sums over draws run in a fixed
 * order on chip (no float atomics): repeated calls are bit-identical. */
#ifndef HODE_SYLVESTER_H_
#define HODE_SYLVESTER_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HODE_SYLVESTER_ABI_VERSION 1
#define HODE_SYLVESTER_MAX_LATENT 32
#define HODE_SYLVESTER_MAX_ORTHO 32
#define HODE_SYLVESTER_MAX_FLOWS 16
#define HODE_SYLVESTER_MAX_SAMPLES 256

#define HODE_SYLVESTER_E_NULL -1      /* a required pointer is NULL */
#define HODE_SYLVESTER_E_SIZE -2      /* struct_size mismatch / dimension outside the domain */
#define HODE_SYLVESTER_E_WORKSPACE -3 /* workspace missing, too small or not 16-byte aligned */

typedef struct hode_sylvester_desc {
  uint32_t struct_size;
  int32_t batch;            /* B */
  int32_t latent_dim;       /* D */
  int32_t n_ortho;          /* M; triangular mode: M == D */
  int32_t n_flows;          /* K */
  int32_t n_samples;        /* S */
  const float* z0;          /* [S][B][D] */
  const float* r1;          /* [B][K][M][M] */
  const float* r2;          /* [B][K][M][M] */
  const float* b;           /* [B][K][M] */
  const float* q;           /* [B][K][D][M]; NULL selects triangular mode */
  const int32_t* perm;      /* [K][D] with entries in 0 .. D-1, triangular mode only, or NULL (identity) */
  float* z_out;             /* forward out [S][B][D] */
  float* logdet;            /* forward out [S][B] */
  float* log_diag;          /* forward out [S][B][K][M], or NULL */
  void* workspace;          /* the tape: forward out (or NULL: no backward will follow), backward in (required if K > 1) */
  size_t workspace_bytes;
  const float* grad_z_out;  /* backward in [S][B][D], or NULL (zero) */
  const float* grad_logdet; /* backward in [S][B], or NULL (zero) */
  const float* grad_log_diag; /* backward in [S][B][K][M], or NULL (zero) */
  float* grad_z0;           /* backward out [S][B][D] (overwritten) */
  float* grad_r1;           /* backward out [B][K][M][M] */
  float* grad_r2;           /* backward out [B][K][M][M] */
  float* grad_b;            /* backward out [B][K][M] */
  float* grad_q;            /* backward out [B][K][D][M]; required in dense mode, ignored in triangular mode */
} hode_sylvester_desc;

int hode_sylvester_version(void);
const char* hode_sylvester_last_error_string(void);
/* bytes of the tape for the descriptor's batch, latent_dim, n_flows and n_samples (0 for K == 1); 0 outside the domain */
size_t hode_sylvester_workspace_bytes(const hode_sylvester_desc* desc);
/* z_out, logdet and (optionally) log_diag; writes the tape when a workspace is given */
int hode_sylvester_fwd(const hode_sylvester_desc* desc, void* hip_stream);
/* reads z0 and the forward's tape; every grad_* output of the mode is required */
int hode_sylvester_bwd(const hode_sylvester_desc* desc, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* HODE_SYLVESTER_H_ */
