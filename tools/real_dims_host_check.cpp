// Stand-alone walk through the host code of libhode_real_dims.so -- the domain check, the workspace layout and the
// dispatch of csrc/real_dims/hode_real_dims.hip, most of it csrc/hode_real_side_host.hpp, which the other two real_*
// side libraries share -- with no GPU and no launch: every call here is refused before the
// dispatch, and the per-hidden-tile launchers are replaced by stubs that abort if one is reached.  Meant for a sanitizer
// build of the host side (from the repository root):
//   hipcc --offload-arch=gfx950 -std=c++17 -g -O1 -Xarch_host -fsanitize=address,undefined -fsanitize=address,undefined \
//       hybrid-ode-neurips-2021_amd/csrc/real_dims/hode_real_dims.hip tools/real_dims_host_check.cpp -o real_dims_host_check
//   ./real_dims_host_check        # prints "real_dims_host_check: N checks ok", exit status 0
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../hybrid-ode-neurips-2021_amd/csrc/real_dims/hode_real_dims.hpp"

namespace hode {
#define HODE_REAL_DIMS_STUB(n)                                                                   \
  int real_dims_launch_ht##n(int, bool, const RealArgs&, int, float*, hipStream_t) {             \
    fprintf(stderr, "real_dims_host_check: the dispatch reached a launch (ht%d)\n", n);          \
    abort();                                                                                     \
  }
HODE_REAL_SIDE_HTS(HODE_REAL_DIMS_STUB)
#undef HODE_REAL_DIMS_STUB
}  // namespace hode

static int n_checks = 0;

static void expect(bool ok, const char* what, int line) {
  ++n_checks;
  if (ok) return;
  fprintf(stderr, "real_dims_host_check: line %d: %s -- last error: %s\n", line, what, hode_real_dims_last_error_string());
  exit(1);
}
#define EXPECT(c) expect((c), #c, __LINE__)

static bool says(const char* text) { return strstr(hode_real_dims_last_error_string(), text) != nullptr; }

static hode_solve_desc base(int D) {
  hode_solve_desc d;
  memset(&d, 0, sizeof(d));
  d.struct_size = sizeof(d);
  d.rhs_kind = HODE_RHS_ROCHE_REAL;
  d.method = HODE_METHOD_RK4_38;
  d.batch = 17; d.latent_dim = D; d.n_times = 6; d.hidden_dim = 43; d.n_action_times = 10;
  return d;
}

static size_t up(size_t n) { return (n + 255) / 256 * 256; }

int main() {
  typedef int (*entry)(const hode_solve_desc*, void*);
  const entry entries[2] = {hode_real_dims_rk_fwd, hode_real_dims_rk_bwd};
  static float buf[64];
  EXPECT(hode_real_dims_version() == HODE_REAL_DIMS_ABI_VERSION);
  const char* sizes = "latent_dim 5 .. 20 with hidden_dim 1 .. 64";
  for (int k = 0; k < 2; ++k) {
    const entry fn = entries[k];
    EXPECT(fn(nullptr, nullptr) == HODE_E_NULL);
    hode_solve_desc d = base(10);
    d.struct_size = 8;
    EXPECT(fn(&d, nullptr) == HODE_E_SIZE && says("struct_size 8"));
    for (int kind = 0; kind < 8; ++kind) {
      if (kind == HODE_RHS_ROCHE_REAL) continue;
      d = base(10); d.rhs_kind = kind;
      EXPECT(fn(&d, nullptr) == HODE_E_UNSUPPORTED && says("rhs_kind") && says(sizes));
    }
    for (int D = -3; D <= 40; ++D) {
      d = base(D);
      const int e = fn(&d, nullptr);
      if (D >= 5 && D <= 20) EXPECT(e == HODE_E_NULL && says("must be non-NULL"));
      else EXPECT(e == HODE_E_UNSUPPORTED && says("latent_dim") && says(sizes) && says("libhode.so has latent_dim 4 and 20"));
    }
    for (int H = -2; H <= 130; ++H) {
      d = base(12); d.hidden_dim = H;
      const int e = fn(&d, nullptr);
      if (H >= 1 && H <= 64) EXPECT(e == HODE_E_NULL);
      else EXPECT(e == HODE_E_UNSUPPORTED && says("hidden_dim") && says(sizes));
    }
    for (int lanes = -1; lanes <= 64; ++lanes) {
      d = base(12); d.lanes_per_patient = lanes;
      const int e = fn(&d, nullptr);
      if (lanes == 0 || lanes == 16) EXPECT(e == HODE_E_NULL);
      else EXPECT(e == HODE_E_UNSUPPORTED && says("lanes_per_patient") && says("matrix-core layout only"));
    }
    for (int m = -1; m <= 5; ++m) {
      d = base(12); d.method = m;
      const int e = fn(&d, nullptr);
      if (m >= HODE_METHOD_EULER && m <= HODE_METHOD_RK4_38) EXPECT(e == HODE_E_NULL);
      else EXPECT(e == HODE_E_UNSUPPORTED && says("method"));
    }
    d = base(12); d.flags = 4;
    EXPECT(fn(&d, nullptr) == HODE_E_UNSUPPORTED && says("flags 4"));
    d = base(12); d.batch = 0;
    EXPECT(fn(&d, nullptr) == HODE_E_SIZE && says("batch=0"));
    d = base(12); d.n_times = -1;
    EXPECT(fn(&d, nullptr) == HODE_E_SIZE && says("n_times=-1"));
    d = base(12); d.n_action_times = 0;
    EXPECT(fn(&d, nullptr) == HODE_E_SIZE && says("n_action_times=0"));
  }
  // pointers, grad_w1, workspace: the last refusals before the dispatch
  hode_solve_desc d = base(19);
  d.t = d.y0 = d.dosage = d.theta = d.w1 = buf;
  d.h = buf;
  EXPECT(hode_real_dims_rk_fwd(&d, nullptr) == HODE_E_WORKSPACE && says("workspace 0 B < required"));
  EXPECT(hode_real_dims_rk_bwd(&d, nullptr) == HODE_E_NULL && says("grad_h / grad_y0 / grad_theta"));
  d.grad_h = buf; d.grad_y0 = buf; d.grad_theta = buf;
  EXPECT(hode_real_dims_rk_bwd(&d, nullptr) == HODE_E_UNSUPPORTED && says("grad_w1 is NULL"));
  d.grad_w1 = buf;
  EXPECT(hode_real_dims_rk_bwd(&d, nullptr) == HODE_E_WORKSPACE);
  d.workspace = (char*)buf + 4;
  d.workspace_bytes = hode_real_dims_workspace_bytes(&d, HODE_WS_RK_BWD);
  EXPECT(hode_real_dims_rk_bwd(&d, nullptr) == HODE_E_ALIGN && says("16-byte aligned"));
  d.workspace_bytes -= 1;
  EXPECT(hode_real_dims_rk_bwd(&d, nullptr) == HODE_E_WORKSPACE);
  // the workspace sizes over the whole domain, against the layout rule restated here; INT_MAX-sized batches do not wrap
  for (int D = 5; D <= 20; ++D)
    for (int H = 1; H <= 64; ++H)
      for (int B : {1, 15, 16, 17, 37, 8192, 2147483647})
        for (int Ta : {1, 30, 120}) {
          hode_solve_desc q = base(D);
          q.hidden_dim = H; q.batch = B; q.n_action_times = Ta;
          const size_t dose = up((size_t)2 * ((size_t)Ta + 1) * (size_t)B * 4), nw = ((size_t)B + 15) / 16, ht = (H + 15) / 16;
          EXPECT(hode_real_dims_workspace_bytes(&q, HODE_WS_RK_FWD) == dose);
          EXPECT(hode_real_dims_workspace_bytes(&q, HODE_WS_RK_BWD) == up(nw * ((4 * ht + 3) * 256 + 16) * 4) + up(nw * 12) + dose);
          EXPECT(hode_real_dims_workspace_bytes(&q, HODE_WS_DOPRI5_FWD) == 0);
        }
  hode_solve_desc bad = base(4);
  EXPECT(hode_real_dims_workspace_bytes(&bad, HODE_WS_RK_BWD) == 0);
  bad = base(12); bad.batch = -5;
  EXPECT(hode_real_dims_workspace_bytes(&bad, HODE_WS_RK_BWD) == 0);
  EXPECT(hode_real_dims_workspace_bytes(nullptr, HODE_WS_RK_BWD) == 0);
  printf("real_dims_host_check: %d checks ok\n", n_checks);
  return 0;
}
