// amgd_mrhs_dev.h -- the row-sum device functions of the K-column kernels (K = 2, 4, 8
// interleaved vectors, element (position q, column j) at q*K + j), shared by the multi-RHS
// V-cycle (amgd_solve_mrhs.hip, where the two families are described) and the K-column level-0
// product of the multi-RHS Krylov solver (amgd_krylov_mrhs.hip).
#ifndef AMGD_MRHS_DEV_H
#define AMGD_MRHS_DEV_H
#include <hip/hip_runtime.h>
#include <stdint.h>

template <int K> struct alignas(16) VecK { double v[K]; };
template <int K> __device__ __forceinline__ VecK<K> ldk(const double *p) {
  return *reinterpret_cast<const VecK<K> *>(p);
}
template <int K> __device__ __forceinline__ void stk(double *p, const VecK<K> &v) {
  *reinterpret_cast<VecK<K> *>(p) = v;
}

// short rows: a block owns VN_ROWS consecutive rows and stages VN_CH (value, column) pairs at a time
#define VN_ROWS 256
#define VN_CH 2048
template <int K>
__device__ __forceinline__ VecK<K> vn_block_rows(double *sa, uint32_t *sc, const uint64_t *ro,
                                                 const uint32_t *col, const double *a, const double *x,
                                                 uint64_t r0, uint64_t r1, uint64_t i, bool own) {
  const int tid = threadIdx.x;
  const uint64_t b0 = ro[r0], b1 = ro[r1];
  const uint64_t k0 = own ? ro[i] : 0, k1 = own ? ro[i + 1] : 0;
  VecK<K> t;
#pragma unroll
  for (int j = 0; j < K; j++) t.v[j] = 0.0;
  for (uint64_t c0 = b0; c0 < b1; c0 += VN_CH) {
    const uint64_t c1 = min(b1, c0 + VN_CH);
    for (uint64_t k = c0 + tid; k < c1; k += VN_ROWS) {
      sa[k - c0] = a[k];
      sc[k - c0] = col[k];
    }
    __syncthreads();
    const uint64_t lo = max(k0, c0), hi = min(k1, c1);
#pragma unroll 2                                // two gathers in flight per thread
    for (uint64_t k = lo; k < hi; k++) {
      const double av = sa[k - c0];
      const VecK<K> xv = ldk<K>(x + (uint64_t)sc[k - c0] * K);
#pragma unroll
      for (int j = 0; j < K; j++) t.v[j] += av * xv.v[j];
    }
    __syncthreads();
  }
  return t;
}
#define VN_BLOCK_LOOP(n)                                                                       \
  for (uint64_t r0 = (uint64_t)blockIdx.x * VN_ROWS; r0 < (n); r0 += (uint64_t)gridDim.x * VN_ROWS)
static inline int vn_block_grid(uint32_t n) {
  const uint64_t g = ((uint64_t)n + VN_ROWS - 1) / VN_ROWS;
  return (int)(g < 1 ? 1 : g > 16384 ? 16384 : g);
}

// long rows: a wavefront owns 64 / K rows, rounds of VN_SEG entries per row
#define VN_SEG 16
template <int K> struct alignas(16) VnTile {
  static constexpr int RW = 64 / K, PER = VN_SEG / K;
  double buf[4][RW][VN_SEG + 1][K];
  uint64_t rk0[4][RW];
  uint32_t rlen[4][RW];
};
__device__ __forceinline__ void vn_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
template <int K>
__device__ __forceinline__ double vn_coop_rows(VnTile<K> &T, const uint64_t *ro, const uint32_t *col,
                                               const double *a, const double *x, uint64_t rb, uint32_t n) {
  constexpr int PER = VnTile<K>::PER;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int lr = lane / K, lj = lane % K;
  const uint64_t r = rb + lr;
  const bool own = r < n;
  const uint64_t k0 = own ? ro[r] : 0, k1 = own ? ro[r + 1] : 0;
  const uint32_t len = (uint32_t)(k1 - k0);
  vn_wave_sync();                          // the previous call's tile reads are done
  if (lj == 0) {
    T.rk0[w][lr] = k0;
    T.rlen[w][lr] = len;
  }
  uint32_t mx = len;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { uint32_t u = __shfl_xor(mx, o, 64); mx = u > mx ? u : mx; }
  vn_wave_sync();
  double t = 0.0;
  for (uint32_t off = 0; off < mx; off += VN_SEG) {
    // all of a round's loads are issued before any is used: a lane past its row's end reads
    // entry 0 (there is one: mx > 0) and drops the product, so no load waits behind a branch
    double av[PER];
    uint32_t cv[PER];
    bool ok[PER];
#pragma unroll
    for (int q = 0; q < PER; q++) {
      const int fl = q * 64 + lane, rr = fl / VN_SEG, sub = fl % VN_SEG;
      const uint32_t en = off + sub;
      ok[q] = en < T.rlen[w][rr];
      const uint64_t k = ok[q] ? T.rk0[w][rr] + en : 0;
      av[q] = a[k];
      cv[q] = col[k];
    }
    VecK<K> xv[PER];
#pragma unroll
    for (int q = 0; q < PER; q++) xv[q] = ldk<K>(x + (uint64_t)cv[q] * K);
#pragma unroll
    for (int q = 0; q < PER; q++) {
      const int fl = q * 64 + lane, rr = fl / VN_SEG, sub = fl % VN_SEG;
      if (ok[q]) {                         // a slot past its row's end is never read
        VecK<K> pr;
#pragma unroll
        for (int j = 0; j < K; j++) pr.v[j] = av[q] * xv[q].v[j];
        stk<K>(&T.buf[w][rr][sub][0], pr);
      }
    }
    vn_wave_sync();
    if (off < len) {
      const uint32_t m = min((uint32_t)VN_SEG, len - off);
      for (uint32_t e = 0; e < m; e++) t += T.buf[w][lr][e][lj];
    }
    vn_wave_sync();
  }
  return t;
}
#define VN_WAVE_LOOP(n)                                                                        \
  for (uint64_t rb = ((uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * (64 / K); rb < (n);     \
       rb += (uint64_t)gridDim.x * 4 * (64 / K))
static inline int vn_wave_grid(uint64_t n, int K) {
  const uint64_t per = 4ull * (64 / K), g = (n + per - 1) / per;
  return (int)(g < 1 ? 1 : g > 65536 ? 65536 : g);
}
#endif
