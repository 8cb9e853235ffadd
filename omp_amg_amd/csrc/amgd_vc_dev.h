// amgd_vc_dev.h -- the device layer under every V-cycle kernel: the three pointwise updates of a
// level, written once, and the four ordered row sums as policy types that the kernel templates
// (amgd_solve.hip) and the K-column level-0 product (amgd_krylov_mrhs.hip) are written over.
// K = 2, 4, 8 interleaved vectors hold element (position q, column j) at q*K + j.
#ifndef AMGD_VC_DEV_H
#define AMGD_VC_DEV_H
#include <hip/hip_runtime.h>
#include <stdint.h>

// ---------------------------------------------------------------------------
// The updates, in the reference's operation order (amg.c:125-126, :142-166).  Every kernel that
// performs one calls these and nothing else; -ffp-contract=off keeps the expressions as written.
// ---------------------------------------------------------------------------
// restriction: bC += t; the last Chebyshev step: xf += v
__device__ __forceinline__ double vc_add(double y, double t) { return y + t; }
// prolongation: bb = bf - tp; cc = D*bb; xf = add ? xw + cc : xw
struct VcPro { double bb, cc, xf; };
__device__ __forceinline__ VcPro vc_prolong(double bf, double tp, double d, double xw, int add) {
  VcPro o;
  o.bb = bf - tp;
  o.cc = d * o.bb;
  o.xf = add ? xw + o.cc : xw;
  return o;
}
// Chebyshev from a given r: v = beta*(c + D*r) [- gamma*cn].  cn comes as a pointer and is read
// under has_prev only: a reference would let the compiler read it ahead of the test
__device__ __forceinline__ double vc_cheb_r(double c, double d, double r, double beta, double gamma,
                                            int has_prev, const double *cn) {
  double v = beta * (c + d * r);
  if (has_prev) v = v - gamma * *cn;
  return v;
}
// Chebyshev from the row sum t of Af against c: r = bf - t
__device__ __forceinline__ double vc_cheb(double bf, double t, double c, double d, double beta, double gamma,
                                          int has_prev, const double *cn) {
  return vc_cheb_r(c, d, bf - t, beta, gamma, has_prev, cn);
}

// N contiguous doubles moved as one piece
template <int N> struct alignas(N == 1 ? 8 : 16) VecK { double v[N]; };
template <int N> __device__ __forceinline__ VecK<N> ldk(const double *p) {
  return *reinterpret_cast<const VecK<N> *>(p);
}
template <int N> __device__ __forceinline__ void stk(double *p, const VecK<N> &v) {
  *reinterpret_cast<VecK<N> *>(p) = v;
}

// ---------------------------------------------------------------------------
// Row-sum policies.  A kernel over policy P runs, with 256 threads a block,
//
//   __shared__ typename P::Shared S;
//   for (uint64_t g = P::first(); g < n; g += P::stride()) {
//     const VecK<P::OWN> t = P::rows(S, ro, col, a, x, g, n);     // every thread calls it
//     if (P::owns(g, n)) ...                     // this thread finishes row P::row(g)
//   }
//
// g: the first row of the group a block (Block forms) or a wavefront (Coop forms) owns.  The
// finishing thread holds the ordered sums -- the products a_ik * x_k added left to right from +0
// -- of the OWN contiguous vector elements from e = P::elem(g) on: of row i = P::row(g) itself
// (Cols == 1), of its K columns (VnBlock), or of its column e - i*K (VnCoop).  grid(n): the
// launch's blocks.
// ---------------------------------------------------------------------------
static inline int vc_grid_of(uint64_t n, uint64_t per, uint64_t cap) {
  const uint64_t g = (n + per - 1) / per;
  return (int)(g < 1 ? 1 : g > cap ? cap : g);
}
__device__ __forceinline__ void vc_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
#define VC_ROWS 256       // rows a block owns in the two Block forms

// One vector, short rows (mean below WAVE_ROWS_MIN_MEAN): one thread adds each row, and the
// loads are shared -- k_spmv's structure (amgd_sparse.hip).  A 256-thread block owns 256
// consecutive rows and walks their entry range in chunks of CH: all threads form the chunk's
// products with coalesced loads of (value, column) into LDS, then each thread adds the part of
// its own row inside the chunk, in order.  Chunks are visited in order, so every row sum is the
// reference's left-to-right sum from +0 whatever the row lengths.  (A plain loop of one thread
// over its row reads the matrix uncoalesced and measured slower than the composed path:
// DESIGN.md "Solve".)
struct VcBlock {
  static constexpr int Cols = 1, OWN = 1, CH = 4096;
  struct Shared { double pv[CH]; };
  static int grid(uint32_t n) { return vc_grid_of(n, VC_ROWS, 16384); }
  static __device__ __forceinline__ uint64_t first() { return (uint64_t)blockIdx.x * VC_ROWS; }
  static __device__ __forceinline__ uint64_t stride() { return (uint64_t)gridDim.x * VC_ROWS; }
  static __device__ __forceinline__ uint64_t row(uint64_t r0) { return r0 + threadIdx.x; }
  static __device__ __forceinline__ uint64_t elem(uint64_t r0) { return row(r0); }
  static __device__ __forceinline__ uint64_t end(uint64_t r0, uint32_t n) { return min((uint64_t)n, r0 + VC_ROWS); }
  static __device__ __forceinline__ bool owns(uint64_t r0, uint32_t n) { return row(r0) < end(r0, n); }
  static __device__ __forceinline__ VecK<1> rows(Shared &S, const uint64_t *ro, const uint32_t *col,
                                                 const double *a, const double *x, uint64_t r0, uint32_t n) {
    double *pv = S.pv;
    const int tid = threadIdx.x;
    const uint64_t r1 = end(r0, n), i = row(r0);
    const bool own = owns(r0, n);
    const uint64_t b0 = ro[r0], b1 = ro[r1];
    const uint64_t k0 = own ? ro[i] : 0, k1 = own ? ro[i + 1] : 0;
    double t = 0.0;
    for (uint64_t c0 = b0; c0 < b1; c0 += CH) {
      const uint64_t c1 = min(b1, c0 + CH);
      for (uint64_t kb = c0 + tid; kb < c1; kb += 256 * 8) {
        double av[8];
        uint32_t cv[8];
#pragma unroll
        for (int u = 0; u < 8; u++) {
          const uint64_t k = kb + 256 * u;
          av[u] = 0.0;
          cv[u] = 0;
          if (k < c1) {
            av[u] = a[k];
            cv[u] = col[k];
          }
        }
#pragma unroll
        for (int u = 0; u < 8; u++) {
          const uint64_t k = kb + 256 * u;
          if (k < c1) pv[k - c0] = av[u] * x[cv[u]];
        }
      }
      __syncthreads();
      const uint64_t lo = max(k0, c0), hi = min(k1, c1);
#pragma unroll 8
      for (uint64_t k = lo; k < hi; k++) t += pv[k - c0];
      __syncthreads();
    }
    return VecK<1>{{t}};
  }
};

// One vector, long rows (mean row >= WAVE_ROWS_MIN_MEAN), after k_spmv_pipe's structure
// (amgd_sparse.hip): a wavefront owns RW rows and walks them in rounds of SEG = 64 PER / RW
// entries per row.  A round's (value, column) pairs are loaded coalesced -- each load
// instruction covers whole row segments -- multiplied with the gathered x and staged in an
// LDS tile; lane r of the first RW then adds row r's segment left to right, so every row
// sum is the reference's ordered sum from +0.  The wavefront-scope fences and barriers
// around the tile are required exactly as there: the tile is written by all 64 lanes and
// read by other lanes of the same wavefront.  Unlike k_spmv_pipe the next round's loads are
// not issued ahead of the adds; a lane past its row's end loads nothing.
// RW by row count like the setup's lane kernel: 4 below 2^16 rows, 16 below 2^22, else 64.
template <int RW, int PER> struct VcCoop {
  static constexpr int Cols = 1, OWN = 1, SEG = 64 * PER / RW;
  struct Shared {
    double buf[4][RW][SEG + 1];
    uint64_t rk0[4][RW];
    uint32_t rlen[4][RW];
  };
  static int grid(uint32_t n) { return vc_grid_of(n, 4 * RW, 65536); }
  static __device__ __forceinline__ uint64_t first() {
    return ((uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * RW;
  }
  static __device__ __forceinline__ uint64_t stride() { return (uint64_t)gridDim.x * 4 * RW; }
  static __device__ __forceinline__ uint64_t row(uint64_t rb) { return rb + (threadIdx.x & 63); }
  static __device__ __forceinline__ uint64_t elem(uint64_t rb) { return row(rb); }
  static __device__ __forceinline__ bool owns(uint64_t rb, uint32_t n) {
    return (threadIdx.x & 63) < RW && row(rb) < n;
  }
  static __device__ __forceinline__ VecK<1> rows(Shared &T, const uint64_t *ro, const uint32_t *col,
                                                 const double *a, const double *x, uint64_t rb, uint32_t n) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint64_t r = rb + lane;
    const bool own = lane < RW && r < n;
    const uint64_t k0 = own ? ro[r] : 0, k1 = own ? ro[r + 1] : 0;
    const uint32_t len = (uint32_t)(k1 - k0);
    vc_wave_sync();                          // the previous call's tile reads are done
    if (lane < RW) {
      T.rk0[w][lane] = k0;
      T.rlen[w][lane] = len;
    }
    uint32_t mx = len;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { uint32_t u = __shfl_xor(mx, o, 64); mx = u > mx ? u : mx; }
    vc_wave_sync();
    double t = 0.0;
    for (uint32_t off = 0; off < mx; off += SEG) {
#pragma unroll
      for (int q = 0; q < PER; q++) {
        const int fl = q * 64 + lane, rr = fl / SEG, sub = fl % SEG;
        const uint32_t en = off + sub;
        double pr = 0.0;
        if (en < T.rlen[w][rr]) {
          const uint64_t k = T.rk0[w][rr] + en;
          pr = a[k] * x[col[k]];
        }
        T.buf[w][rr][sub] = pr;
      }
      vc_wave_sync();
      if (lane < RW && off < len) {
        const uint32_t m = min((uint32_t)SEG, len - off);
        for (uint32_t e = 0; e < m; e++) t += T.buf[w][lane][e];
      }
      vc_wave_sync();
    }
    return VecK<1>{{t}};
  }
};

// K vectors, short rows.  VcBlock stages the chunk's PRODUCTS in LDS, which would take K times
// its 32 KB here; this form stages the chunk's (value, column) pairs instead (12 B per entry,
// 24 KB a block: no more LDS than one vector takes) and the row's thread forms its K products
// from one contiguous read of x[col*K .. col*K + K).  Chunks in order and entries in order
// inside a chunk: the ordered sum per column, whatever the row lengths.
template <int K> struct VnBlock {
  static constexpr int Cols = K, OWN = K, CH = 2048;
  struct Shared {
    double sa[CH];
    uint32_t sc[CH];
  };
  static int grid(uint32_t n) { return vc_grid_of(n, VC_ROWS, 16384); }
  static __device__ __forceinline__ uint64_t first() { return (uint64_t)blockIdx.x * VC_ROWS; }
  static __device__ __forceinline__ uint64_t stride() { return (uint64_t)gridDim.x * VC_ROWS; }
  static __device__ __forceinline__ uint64_t row(uint64_t r0) { return r0 + threadIdx.x; }
  static __device__ __forceinline__ uint64_t elem(uint64_t r0) { return row(r0) * K; }
  static __device__ __forceinline__ uint64_t end(uint64_t r0, uint32_t n) { return min((uint64_t)n, r0 + VC_ROWS); }
  static __device__ __forceinline__ bool owns(uint64_t r0, uint32_t n) { return row(r0) < end(r0, n); }
  static __device__ __forceinline__ VecK<K> rows(Shared &S, const uint64_t *ro, const uint32_t *col,
                                                 const double *a, const double *x, uint64_t r0, uint32_t n) {
    double *sa = S.sa;
    uint32_t *sc = S.sc;
    const int tid = threadIdx.x;
    const uint64_t r1 = end(r0, n), i = row(r0);
    const bool own = owns(r0, n);
    const uint64_t b0 = ro[r0], b1 = ro[r1];
    const uint64_t k0 = own ? ro[i] : 0, k1 = own ? ro[i + 1] : 0;
    VecK<K> t;
#pragma unroll
    for (int j = 0; j < K; j++) t.v[j] = 0.0;
    for (uint64_t c0 = b0; c0 < b1; c0 += CH) {
      const uint64_t c1 = min(b1, c0 + CH);
      for (uint64_t k = c0 + tid; k < c1; k += VC_ROWS) {
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
};

// K vectors, long rows, after VcCoop: a wavefront owns RW = 64 / K rows and walks them in rounds
// of SEG = 16 entries per row.  A round's 64 * SEG / K (value, column) pairs are loaded
// coalesced, SEG / K per lane, all loads in flight together; each is multiplied with its K
// operands, gathered by one 8K-byte read, and the K products staged in an LDS tile.  Then lane
// r*K + j adds column j of row r's segment left to right: the ordered adds run on all 64 lanes,
// one per (row, column) pair, where the single-vector form has RW lanes adding and the rest
// idle.  The tile is 64 * 17 * 8 B a wavefront whatever K (VcCoop's size at RW = 64); a row is
// padded by one entry slot, so the adding lanes of a 32-lane group read 32 distinct banks.  A
// row of any length is walked in rounds.  Lane r*K + j returns the sum of row rb + r, column j:
// its flat index rb*K + lane is contiguous over the wavefront.
template <int K> struct VnCoop {
  static constexpr int Cols = K, OWN = 1, SEG = 16, RW = 64 / K, PER = SEG / K;
  struct alignas(16) Shared {
    double buf[4][RW][SEG + 1][K];
    uint64_t rk0[4][RW];
    uint32_t rlen[4][RW];
  };
  static int grid(uint32_t n) { return vc_grid_of(n, 4 * RW, 65536); }
  static __device__ __forceinline__ uint64_t first() {
    return ((uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * RW;
  }
  static __device__ __forceinline__ uint64_t stride() { return (uint64_t)gridDim.x * 4 * RW; }
  static __device__ __forceinline__ uint64_t row(uint64_t rb) { return rb + (threadIdx.x & 63) / K; }
  static __device__ __forceinline__ uint64_t elem(uint64_t rb) { return rb * K + (threadIdx.x & 63); }
  static __device__ __forceinline__ bool owns(uint64_t rb, uint32_t n) { return row(rb) < n; }
  static __device__ __forceinline__ VecK<1> rows(Shared &T, const uint64_t *ro, const uint32_t *col,
                                                 const double *a, const double *x, uint64_t rb, uint32_t n) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int lr = lane / K, lj = lane % K;
    const uint64_t r = rb + lr;
    const bool own = r < n;
    const uint64_t k0 = own ? ro[r] : 0, k1 = own ? ro[r + 1] : 0;
    const uint32_t len = (uint32_t)(k1 - k0);
    vc_wave_sync();                          // the previous call's tile reads are done
    if (lj == 0) {
      T.rk0[w][lr] = k0;
      T.rlen[w][lr] = len;
    }
    uint32_t mx = len;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { uint32_t u = __shfl_xor(mx, o, 64); mx = u > mx ? u : mx; }
    vc_wave_sync();
    double t = 0.0;
    for (uint32_t off = 0; off < mx; off += SEG) {
      // all of a round's loads are issued before any is used: a lane past its row's end reads
      // entry 0 (there is one: mx > 0) and drops the product, so no load waits behind a branch
      double av[PER];
      uint32_t cv[PER];
      bool ok[PER];
#pragma unroll
      for (int q = 0; q < PER; q++) {
        const int fl = q * 64 + lane, rr = fl / SEG, sub = fl % SEG;
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
        const int fl = q * 64 + lane, rr = fl / SEG, sub = fl % SEG;
        if (ok[q]) {                         // a slot past its row's end is never read
          VecK<K> pr;
#pragma unroll
          for (int j = 0; j < K; j++) pr.v[j] = av[q] * xv[q].v[j];
          stk<K>(&T.buf[w][rr][sub][0], pr);
        }
      }
      vc_wave_sync();
      if (off < len) {
        const uint32_t m = min((uint32_t)SEG, len - off);
        for (uint32_t e = 0; e < m; e++) t += T.buf[w][lr][e][lj];
      }
      vc_wave_sync();
    }
    return VecK<1>{{t}};
  }
};
#endif
