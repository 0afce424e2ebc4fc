/* C ABI of libhode_flow.so: the planar normalizing-flow posterior (reference flow.py:8-59 Planar, model.py:48-153
 * EncoderPlanarLSTM.reparameterize / log_density, model.py:41-45 ExponentialPrior) with its Monte-Carlo KL, forward and
 * backward, one launch each, gfx950.
 *
 * Per patient b and sample s (eps = noise[s][b][:]):
 *     z0      = eps * exp(0.5 log_var) + mu
 *     for k in 0 .. K-1:   uw = w_k . u_k,  m = -1 + softplus(uw)   (torch softplus: x > 20 -> x)
 *                          u_hat = u_k + (m - uw) w_k / |w_k|^2
 *                          a = w_k . z + b_k;  z = z + u_hat tanh(a);  logdet += log|1 + (1 - tanh(a)^2) w_k . u_hat|
 *     z_out   = exp(z - 5);  logdet += sum_d (z - 5)
 *     kl_s    = sum_d log N(z0; mu, exp(0.5 log_var)) - logdet - sum_d (log 100 - 100 z_out)
 *     kl[b]   = mean over s in [s_kl, S) of kl_s
 *
 * Conventions as in hode.h: row-major float32 device pointers, return 0 on success, <0 an argument error
 * (HODE_FLOW_E_*), >0 a hipError_t from the launch; the message is in hode_flow_last_error_string().
 * Domain: latent_dim 1 .. HODE_FLOW_MAX_LATENT, n_flows 1 .. HODE_FLOW_MAX_FLOWS, n_samples 1 .. HODE_FLOW_MAX_SAMPLES,
 * batch >= 1.  Sums over samples run in a fixed order on chip (no float atomics): repeated calls are bit-identical. */
#ifndef HODE_FLOW_H_
#define HODE_FLOW_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HODE_FLOW_ABI_VERSION 1
#define HODE_FLOW_MAX_LATENT 32
#define HODE_FLOW_MAX_FLOWS 16
#define HODE_FLOW_MAX_SAMPLES 256

#define HODE_FLOW_E_NULL -1 /* a required pointer is NULL */
#define HODE_FLOW_E_SIZE -2 /* struct_size mismatch / dimension outside the domain */

typedef struct hode_flow_desc {
  uint32_t struct_size;
  int32_t batch;          /* B */
  int32_t latent_dim;     /* D */
  int32_t n_flows;        /* K */
  int32_t n_samples;      /* S */
  int32_t s_kl;           /* first sample of the KL mean: 1 (sample 0 is the decoder's draw) or 0; s_kl < S when kl / grad_kl is given */
  const float* mu;        /* [B][D] */
  const float* log_var;   /* [B][D] */
  const float* u;         /* [B][K][D] */
  const float* w;         /* [B][K][D] */
  const float* b;         /* [B][K] */
  const float* noise;     /* [S][B][D] standard-normal draws */
  float* z_out;           /* forward out [S][B][D], or NULL */
  float* kl;              /* forward out [B], or NULL */
  const float* grad_z_out; /* backward in [S][B][D], or NULL (zero) */
  const float* grad_kl;   /* backward in [B], or NULL (zero) */
  float* grad_mu;         /* backward out [B][D] (overwritten) */
  float* grad_log_var;    /* backward out [B][D] */
  float* grad_u;          /* backward out [B][K][D] */
  float* grad_w;          /* backward out [B][K][D] */
  float* grad_b;          /* backward out [B][K] */
} hode_flow_desc;

int hode_flow_version(void);
const char* hode_flow_last_error_string(void);
/* z_out and / or kl; at least one of them */
int hode_flow_fwd(const hode_flow_desc* desc, void* hip_stream);
/* recomputes the forward in registers (no tape); every grad_* output is required */
int hode_flow_bwd(const hode_flow_desc* desc, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* HODE_FLOW_H_ */
