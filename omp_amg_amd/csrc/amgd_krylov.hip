// amgd_krylov.hip -- the orthogonalisation kernels of the flexible GMRES around the V-cycle
// (driver amgd_krylov.c; DESIGN.md "Krylov").  A basis block is column-major: vector t starts
// at V + t*ld, ld >= n, ld of either parity.
//
//   k_kry_mdot    all nb dots v_t . w of a Gram-Schmidt pass in one sweep over w and the basis:
//                 KRY_TILE vectors per workgroup row (blockIdx.y), one partial per workgroup
//                 and vector, every sum in a fixed order (no floating-point atomics)
//   k_kry_fin     the partials of a vector added in a fixed order; optionally the Hessenberg
//                 entry d + d' or the norm sqrt(sum) beside the sum
//   k_kry_axpys   w = ((w -/+ c_0 v_0) -/+ c_1 v_1) ... per element in one pass, the
//                 coefficients read from device memory; optionally the partials of ||w||^2
//   k_kry_scale   v = w / *h
//   k_kry_comb    the ranks' sums of a row-partitioned solve added in rank order, with k_kry_fin's
//                 Hessenberg entry or root
//
// Compiled with -ffp-contract=off: every product is rounded before it is added.
#include <hip/hip_runtime.h>
#include <string.h>
#include <algorithm>

#include "amgd.h"
#include "amgd_dev.h"

// Vectors per workgroup row of k_kry_mdot.  16 accumulators are 32 VGPRs; with the loads of a
// step the kernel takes 46, which keeps eight wavefronts per SIMD resident (DESIGN.md "Krylov"
// has the table); w is re-read once per tile, 1/16 of the basis traffic.
#define KRY_TILE 16
#define KRY_THREADS 256
#define KRY_GRID_MAX 1024

extern "C" int amgd_kry_tile(void) { return KRY_TILE; }
// workgroups per row of the multi-dot: a function of n alone, so the order of every sum is
extern "C" int amgd_kry_grid(uint64_t n) {
  const uint64_t b = (n + 4 * KRY_THREADS - 1) / (4 * KRY_THREADS);
  return (int)std::min<uint64_t>(std::max<uint64_t>(b, 1), KRY_GRID_MAX);
}

// the workgroup's sum of one value per thread, in a fixed order: the shuffle tree inside a
// wavefront, then the wavefronts' sums left to right (valid in thread 0)
__device__ __forceinline__ double kry_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = v + __shfl_down(v, o, 64);
  return v;
}

// PAIR: w and every column are 16-byte aligned (ld even): two elements per load
// (the bodies are __device__ functions: the single kernels and the forms that serve several
// columns in one launch, further down, run the same code on the same grid in x and y)
template <bool PAIR>
__device__ __forceinline__ void kry_mdot_body(double (*s_sum)[KRY_TILE], const double *__restrict__ V, uint64_t ld,
                                              const double *__restrict__ w, uint64_t n, int nb,
                                              double *__restrict__ part) {
  const int v0 = blockIdx.y * KRY_TILE;
  const int nv = min(KRY_TILE, nb - v0);
  const double *B = V + (uint64_t)v0 * ld;
  double acc[KRY_TILE];
#pragma unroll
  for (int t = 0; t < KRY_TILE; t++) acc[t] = 0.;
  if (PAIR) {
    const uint64_t np = n >> 1;
    const double2 *w2 = (const double2 *)w;
    GRID_STRIDE(p, np) {
      const double2 x = w2[p];
#pragma unroll
      for (int t = 0; t < KRY_TILE; t++)
        if (t < nv) {
          const double2 y = ((const double2 *)(B + (uint64_t)t * ld))[p];
          acc[t] = acc[t] + y.x * x.x;
          acc[t] = acc[t] + y.y * x.y;
        }
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
      const double x = w[n - 1];
#pragma unroll
      for (int t = 0; t < KRY_TILE; t++)
        if (t < nv) acc[t] = acc[t] + B[(uint64_t)t * ld + n - 1] * x;
    }
  } else {
    GRID_STRIDE(i, n) {
      const double x = w[i];
#pragma unroll
      for (int t = 0; t < KRY_TILE; t++)
        if (t < nv) acc[t] = acc[t] + B[(uint64_t)t * ld + i] * x;
    }
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int t = 0; t < KRY_TILE; t++) {
    const double s = kry_wave_sum(acc[t]);
    if (lane == 0) s_sum[wv][t] = s;
  }
  __syncthreads();
  if ((int)threadIdx.x < nv) {
    double s = s_sum[0][threadIdx.x];
    for (int q = 1; q < KRY_THREADS / 64; q++) s = s + s_sum[q][threadIdx.x];
    part[(uint64_t)(v0 + threadIdx.x) * gridDim.x + blockIdx.x] = s;
  }
}
template <bool PAIR>
__global__ __launch_bounds__(KRY_THREADS) void k_kry_mdot(const double *__restrict__ V, uint64_t ld,
                                                          const double *__restrict__ w, uint64_t n, int nb,
                                                          double *__restrict__ part) {
  __shared__ double s_sum[KRY_THREADS / 64][KRY_TILE];
  kry_mdot_body<PAIR>(s_sum, V, ld, w, n, nb, part);
}

// block b: out[b] = the G partials of vector b, thread t taking t, t + 256, ... then the
// workgroup's fixed tree.  prev: hsum[b] = prev[b] + out[b] (the Hessenberg entry of classical
// Gram-Schmidt applied twice); root: root[0] = sqrt(out[0])
__device__ __forceinline__ void kry_fin_body(double *s_sum, const double *__restrict__ part, int G,
                                             double *__restrict__ out, const double *prev, double *hsum,
                                             double *root) {
  const double *p = part + (uint64_t)blockIdx.x * G;
  double s = 0.;
  for (int q = threadIdx.x; q < G; q += KRY_THREADS) s = s + p[q];
  s = kry_wave_sum(s);
  if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double r = s_sum[0];
    for (int q = 1; q < KRY_THREADS / 64; q++) r = r + s_sum[q];
    out[blockIdx.x] = r;
    if (prev) hsum[blockIdx.x] = prev[blockIdx.x] + r;
    if (root) root[0] = sqrt(r);
  }
}
__global__ __launch_bounds__(KRY_THREADS) void k_kry_fin(const double *__restrict__ part, int G,
                                                         double *__restrict__ out, const double *prev,
                                                         double *hsum, double *root) {
  __shared__ double s_sum[KRY_THREADS / 64];
  kry_fin_body(s_sum, part, G, out, prev, hsum, root);
}

// ADD 0: w -= c_t v_t, 1: w += c_t v_t, t ascending, each product rounded and formed whatever
// the coefficient (0 * inf gives NaN as on the host).  part != NULL: the workgroup's partial
// of the sum of the new w's squares at part[blockIdx.x] (every workgroup writes one)
template <bool ADD, bool PAIR>
__device__ __forceinline__ void kry_axpys_body(double *s_sum, double *__restrict__ w, const double *__restrict__ V,
                                               uint64_t ld, const double *__restrict__ c, int nb, uint64_t n,
                                               double *__restrict__ part) {
  double sq = 0.;
  if (PAIR) {
    const uint64_t np = n >> 1;
    double2 *w2 = (double2 *)w;
    GRID_STRIDE(p, np) {
      double2 x = w2[p];
      int t = 0;
      for (; t + 4 <= nb; t += 4) {                      /* four columns' loads in flight */
        double2 y[4];
#pragma unroll
        for (int q = 0; q < 4; q++) y[q] = ((const double2 *)(V + (uint64_t)(t + q) * ld))[p];
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const double cq = c[t + q];
          x.x = ADD ? x.x + cq * y[q].x : x.x - cq * y[q].x;
          x.y = ADD ? x.y + cq * y[q].y : x.y - cq * y[q].y;
        }
      }
      for (; t < nb; t++) {
        const double2 y = ((const double2 *)(V + (uint64_t)t * ld))[p];
        const double cq = c[t];
        x.x = ADD ? x.x + cq * y.x : x.x - cq * y.x;
        x.y = ADD ? x.y + cq * y.y : x.y - cq * y.y;
      }
      w2[p] = x;
      sq = sq + x.x * x.x;
      sq = sq + x.y * x.y;
    }
  }
  // the unpaired form; after the pairs: the last element of an odd n
  const uint64_t first = PAIR ? (n & ~(uint64_t)1) : 0;
  for (uint64_t i = first + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * blockDim.x) {
    double x = w[i];
    for (int t = 0; t < nb; t++) {
      const double cq = c[t], y = V[(uint64_t)t * ld + i];
      x = ADD ? x + cq * y : x - cq * y;
    }
    w[i] = x;
    sq = sq + x * x;
  }
  if (part) {
    sq = kry_wave_sum(sq);
    if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = sq;
    __syncthreads();
    if (threadIdx.x == 0) {
      double r = s_sum[0];
      for (int q = 1; q < KRY_THREADS / 64; q++) r = r + s_sum[q];
      part[blockIdx.x] = r;
    }
  }
}
template <bool ADD, bool PAIR>
__global__ __launch_bounds__(KRY_THREADS) void k_kry_axpys(double *__restrict__ w, const double *__restrict__ V,
                                                           uint64_t ld, const double *__restrict__ c, int nb,
                                                           uint64_t n, double *__restrict__ part) {
  __shared__ double s_sum[KRY_THREADS / 64];
  kry_axpys_body<ADD, PAIR>(s_sum, w, V, ld, c, nb, n, part);
}

__device__ __forceinline__ void kry_scale_body(double *__restrict__ v, const double *__restrict__ w,
                                               const double *__restrict__ h, uint64_t n) {
  const double d = h[0];
  GRID_STRIDE(i, n) v[i] = w[i] / d;
}
__global__ void k_kry_scale(double *__restrict__ v, const double *__restrict__ w, const double *__restrict__ h,
                            uint64_t n) {
  kry_scale_body(v, w, h, n);
}

static bool kry_pair(const void *a, const void *b, uint64_t ld) {
  return (((uintptr_t)a | (uintptr_t)b) & 15) == 0 && (ld & 1) == 0;
}

// d[t] = v_t . w for t < nb (nb >= 1); part: nb * amgd_kry_grid(n) doubles.  prev / hsum /
// root: see k_kry_fin (root only with nb == 1)
extern "C" void amgd_kry_mdot(const double *V, uint64_t ld, const double *w, uint64_t n, int nb, double *part,
                              double *d, const double *prev, double *hsum) {
  if (nb < 1) return;
  const int G = amgd_kry_grid(n);
  const dim3 grid(G, (nb + KRY_TILE - 1) / KRY_TILE);
  if (kry_pair(V, w, ld)) k_kry_mdot<true><<<grid, KRY_THREADS, 0, amgd_s()>>>(V, ld, w, n, nb, part);
  else k_kry_mdot<false><<<grid, KRY_THREADS, 0, amgd_s()>>>(V, ld, w, n, nb, part);
  k_kry_fin<<<nb, KRY_THREADS, 0, amgd_s()>>>(part, G, d, prev, hsum, nullptr);
  KCHECK();
  amgd_route_hit(AMGD_R_KRY_MDOT);
}
// w = ((w -/+ c_0 v_0) -/+ ...) with c on the device; nrm2 != NULL: nrm2[0] = the sum of the
// new w's squares (fixed order) and root[0] = its square root; part: amgd_kry_grid(n) doubles
extern "C" void amgd_kry_axpys(double *w, const double *V, uint64_t ld, const double *c, int nb, uint64_t n, int add,
                               double *part, double *nrm2, double *root) {
  const int G = amgd_kry_grid(n);
  double *pp = nrm2 ? part : nullptr;
  const bool pair = kry_pair(V, w, ld);
  hipStream_t st = amgd_s();
  if (add) {
    if (pair) k_kry_axpys<true, true><<<G, KRY_THREADS, 0, st>>>(w, V, ld, c, nb, n, pp);
    else k_kry_axpys<true, false><<<G, KRY_THREADS, 0, st>>>(w, V, ld, c, nb, n, pp);
  } else {
    if (pair) k_kry_axpys<false, true><<<G, KRY_THREADS, 0, st>>>(w, V, ld, c, nb, n, pp);
    else k_kry_axpys<false, false><<<G, KRY_THREADS, 0, st>>>(w, V, ld, c, nb, n, pp);
  }
  if (nrm2) k_kry_fin<<<1, KRY_THREADS, 0, st>>>(part, G, nrm2, nullptr, nullptr, root);
  KCHECK();
}
extern "C" void amgd_kry_scale(double *v, const double *w, const double *h, uint64_t n) {
  if (n) k_kry_scale<<<grid_for(n), 256, 0, amgd_s()>>>(v, w, h, n);
}

// Several ranks (a row-partitioned hierarchy): every rank ran k_kry_mdot / k_kry_fin on its own
// rows, g holds rank r's nb sums at g + r*nb on every rank.  Thread t adds sum t in rank order,
// s = p_0; s = s + p_1; ..., and applies what k_kry_fin applies on one GPU: the Hessenberg
// entry prev + s, or the square root behind the sum.  nb <= AMGD_KRYLOV_MAX_RESTART + 1: one
// workgroup.
__global__ __launch_bounds__(KRY_THREADS) void k_kry_comb(const double *__restrict__ g, int np, int nb,
                                                          double *__restrict__ out, const double *prev,
                                                          double *hsum, double *root) {
  const int t = threadIdx.x;
  if (t >= nb) return;
  double s = g[t];
  for (int r = 1; r < np; r++) s = s + g[(uint64_t)r * nb + t];
  out[t] = s;
  if (prev) hsum[t] = prev[t] + s;
  if (root && t == 0) root[0] = sqrt(s);
}
extern "C" void amgd_kry_comb(const double *g, int np, int nb, double *out, const double *prev, double *hsum,
                              double *root) {
  if (nb < 1 || nb > KRY_THREADS || np < 1) return;
  k_kry_comb<<<1, KRY_THREADS, 0, amgd_s()>>>(g, np, nb, out, prev, hsum, root);
  KCHECK();
}

// ---------------------------------------------------------------------------
// Several columns in one launch (amgd_krylov_device_n): the column is the grid's last
// dimension, its operands come from a by-value table.  x and y of the grid, the tile loop and
// the paired / unpaired choice per column are the single forms', so every column's sums come
// out in the single kernels' order.
// ---------------------------------------------------------------------------
struct KryTab {
  amgd_kry_col c[8];
  unsigned pair;         // bit q: column q takes the paired form
};
__global__ __launch_bounds__(KRY_THREADS) void k_kry_mdot_n(KryTab T, uint64_t ld, uint64_t n) {
  __shared__ double s_sum[KRY_THREADS / 64][KRY_TILE];
  const amgd_kry_col &c = T.c[blockIdx.z];
  if ((int)blockIdx.y * KRY_TILE >= c.nb) return;
  if ((T.pair >> blockIdx.z) & 1) kry_mdot_body<true>(s_sum, c.V, ld, c.w, n, c.nb, c.part);
  else kry_mdot_body<false>(s_sum, c.V, ld, c.w, n, c.nb, c.part);
}
// after the multi-dot (norm 0): block (t, q) adds vector t's partials of column q; after the
// update (norm 1): block (0, q) adds the partials of ||w||^2
__global__ __launch_bounds__(KRY_THREADS) void k_kry_fin_n(KryTab T, int G, int norm) {
  __shared__ double s_sum[KRY_THREADS / 64];
  const amgd_kry_col &c = T.c[blockIdx.y];
  if (norm) {
    if (blockIdx.x == 0 && c.nrm2) kry_fin_body(s_sum, c.part, G, c.nrm2, nullptr, nullptr, c.root);
  } else if ((int)blockIdx.x < c.nb) {
    kry_fin_body(s_sum, c.part, G, c.d, c.prev, c.hsum, nullptr);
  }
}
__global__ __launch_bounds__(KRY_THREADS) void k_kry_axpys_n(KryTab T, uint64_t ld, uint64_t n) {
  __shared__ double s_sum[KRY_THREADS / 64];
  const amgd_kry_col &c = T.c[blockIdx.y];
  double *pp = c.nrm2 ? c.part : nullptr;
  if ((T.pair >> blockIdx.y) & 1) kry_axpys_body<false, true>(s_sum, c.w, c.V, ld, c.d, c.nb, n, pp);
  else kry_axpys_body<false, false>(s_sum, c.w, c.V, ld, c.d, c.nb, n, pp);
}
__global__ void k_kry_scale_n(KryTab T, uint64_t n) {
  const amgd_kry_col &c = T.c[blockIdx.y];
  kry_scale_body(c.vout, c.w, c.h, n);
}
static KryTab kry_tab(const amgd_kry_col *c, int nc, uint64_t ld, int *maxnb) {
  KryTab T;
  memset(&T, 0, sizeof T);
  int mx = 0;
  for (int q = 0; q < nc; q++) {
    T.c[q] = c[q];
    if (kry_pair(c[q].V, c[q].w, ld)) T.pair |= 1u << q;
    mx = std::max(mx, c[q].nb);
  }
  if (maxnb) *maxnb = mx;
  return T;
}
// column q: d[t] = v_t . w for t < nb (amgd_kry_mdot's arguments per column)
extern "C" void amgd_kry_mdot_n(const amgd_kry_col *c, int nc, uint64_t ld, uint64_t n) {
  if (nc < 1 || nc > 8) return;
  int mx;
  const KryTab T = kry_tab(c, nc, ld, &mx);
  if (mx < 1) return;
  const int G = amgd_kry_grid(n);
  k_kry_mdot_n<<<dim3(G, (mx + KRY_TILE - 1) / KRY_TILE, nc), KRY_THREADS, 0, amgd_s()>>>(T, ld, n);
  k_kry_fin_n<<<dim3(mx, nc), KRY_THREADS, 0, amgd_s()>>>(T, G, 0);
  KCHECK();
  amgd_route_hit(AMGD_R_KRY_MDOT);
}
// column q: w = ((w - d_0 v_0) - d_1 v_1) ...; nrm2 / root as in amgd_kry_axpys
extern "C" void amgd_kry_axpys_n(const amgd_kry_col *c, int nc, uint64_t ld, uint64_t n) {
  if (nc < 1 || nc > 8) return;
  const KryTab T = kry_tab(c, nc, ld, nullptr);
  const int G = amgd_kry_grid(n);
  bool norm = false;
  for (int q = 0; q < nc; q++) norm = norm || c[q].nrm2;
  k_kry_axpys_n<<<dim3(G, nc), KRY_THREADS, 0, amgd_s()>>>(T, ld, n);
  if (norm) k_kry_fin_n<<<dim3(1, nc), KRY_THREADS, 0, amgd_s()>>>(T, G, 1);
  KCHECK();
}
extern "C" void amgd_kry_scale_n(const amgd_kry_col *c, int nc, uint64_t n) {
  if (nc < 1 || nc > 8 || !n) return;
  const KryTab T = kry_tab(c, nc, 0, nullptr);
  k_kry_scale_n<<<dim3(grid_for(n), nc), 256, 0, amgd_s()>>>(T, n);
  KCHECK();
}
