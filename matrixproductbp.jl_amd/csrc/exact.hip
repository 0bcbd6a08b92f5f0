// Exact solvers (reference src/exact.jl): the ground truth MPBP is validated against.  C ABI: mpbp_exact_* in
// include/mpbp_hip.h.  Two methods that share only the dense transition tables of the context's factors:
//   0  joint enumeration (src/exact.jl:5-41): log p of all Q = prod_i q_i^(T+1) trajectories, normalised on the device,
//      and the strided reductions of p behind site / edge trajectory marginals (src/exact.jl:43-58, 85-100);
//   1  forward-backward over the global state s of all nodes at one time (S = prod_i q_i states): exact on any graph at
//      any T for S <= 2^16.  The transfer matrix K_t(s -> s') = prod_i W_i^t(s'_i | s) is never formed: the nodes are
//      split in two halves, KA[s, s'_A] and KB[s, s'_B] are built once per time block, and a step is one fp64 GEMM.
//      Two-time and alternate marginals carry many conditioned vectors through K at once (k_tt_step, fp64 MFMA).
// Every sum runs in a fixed order that depends on the problem sizes only - workgroup partials over fixed-size chunks,
// then one final pass - and there are no floating-point atomics: results do not depend on the launch geometry.
#include "ctx.h"

#include <cmath>
#include <cstdlib>
#include <limits>

namespace ex {

constexpr int MAXQ = 4;                  // states per variable: a digit of a configuration is held in two bits
constexpr int NT = 256;                  // threads per workgroup of every kernel here
constexpr int CH = 4096;                 // elements of one reduction chunk (fixed: the summation order follows from it)
constexpr int TS = 64, KS = 16;          // output tile and k-step of the two transfer GEMMs (16 x 16 threads, 4 x 4 each)
constexpr int64_t MAX_TABLE = int64_t(1) << 26;   // doubles of one node's dense table per time block
constexpr uint64_t MAX_Q = uint64_t(1) << 32;     // configurations of the enumeration
constexpr int MAX_DIGITS = 64;
constexpr int MAX_S = 1 << 16;           // global states of the transfer method

struct Node {
  int32_t deg, nt, qi, pad;
  int64_t tab_base, tstride;             // dense table [nt][x' + q (x_i + q (x_1 + q (x_2 + ...)))]
};

__device__ inline double ninf() { return -std::numeric_limits<double>::infinity(); }

// fixed-order tree over the NT values of a workgroup (result in red[0])
__device__ inline void tree_sum(double* red) {
  __syncthreads();
  for (int w = NT / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
}
__device__ inline void tree_max(double* red) {
  __syncthreads();
  for (int w = NT / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + w]);
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------ method 0: enumeration
__device__ inline int digit(uint64_t lo, uint64_t hi, int d) { return (int)(((d < 32 ? lo : hi) >> (2 * (d & 31))) & 3); }

// log p (unnormalised) of every configuration and the maximum of each chunk of CH configurations.  Index layout: digit
// d = i L + t, node-major with time inside, the last node's last time fastest (a C-ordered array [q_0]*L + [q_1]*L + ...).
__global__ void __launch_bounds__(NT) k_logp(const Node* __restrict__ nodes, const double* __restrict__ logw,
                                             const int32_t* __restrict__ nbr_ptr, const int32_t* __restrict__ nbr,
                                             const int32_t* __restrict__ in_edge, const double* __restrict__ logphi,
                                             const double* __restrict__ hlpsi, int N, int L, int q, int periodic,
                                             uint64_t Q, uint64_t nchunks, double* __restrict__ logp, double* __restrict__ pmax) {
  __shared__ double red[NT];
  for (uint64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    double m = ninf();
    for (int k = 0; k < CH / NT; k++) {
      const uint64_t idx = c * CH + (uint64_t)k * NT + threadIdx.x;
      if (idx >= Q) break;
      uint64_t lo = 0, hi = 0;
      uint32_t r = (uint32_t)idx;
      for (int i = N - 1; i >= 0; i--) {
        const uint32_t qi = (uint32_t)nodes[i].qi;
        for (int t = L - 1; t >= 0; t--) {
          const uint32_t nr = r / qi;
          const uint64_t x = r - nr * qi;
          r = nr;
          const int d = i * L + t;
          if (d < 32) lo |= x << (2 * d); else hi |= x << (2 * (d - 32));
        }
      }
      double acc = 0.0;
      for (int i = 0; i < N; i++) {
        const Node nd = nodes[i];
        const int pb = nbr_ptr[i], pe = nbr_ptr[i + 1];
        for (int t = 0; t < L; t++) {
          const int x = digit(lo, hi, i * L + t);
          acc += logphi[((size_t)i * L + t) * q + x];
          for (int p = pb; p < pe; p++)        // in-edge nbr -> i: psi[e][t][x_nbr][x_i]
            acc += hlpsi[(((size_t)in_edge[p] * L + t) * q + x) * q + digit(lo, hi, nbr[p] * L + t)];
          if (t + 1 < L || periodic) {
            // W_i^t(x^{t+1} | x_nbrs^t, x^t); the closing factor of a periodic chain is block T and leads back to x^0
            int64_t col = 0;
            for (int p = pe - 1; p >= pb; p--) col = col * q + digit(lo, hi, nbr[p] * L + t);
            col = (col * q + x) * q + digit(lo, hi, i * L + (t + 1 < L ? t + 1 : 0));
            acc += logw[nd.tab_base + (nd.nt > 1 ? (int64_t)t * nd.tstride : 0) + col];
          }
        }
      }
      logp[idx] = acc;
      m = fmax(m, acc);
    }
    red[threadIdx.x] = m;
    tree_max(red);
    if (threadIdx.x == 0) pmax[c] = red[0];
    __syncthreads();
  }
}

// one workgroup: out[0] = max (op 0) or sum (op 1) of in[0..n), strided over the threads, then the tree
__global__ void __launch_bounds__(NT) k_reduce1(const double* __restrict__ in, uint64_t n, int op, double* __restrict__ out) {
  __shared__ double red[NT];
  double a = op == 0 ? ninf() : 0.0;
  for (uint64_t k = threadIdx.x; k < n; k += NT) a = op == 0 ? fmax(a, in[k]) : a + in[k];
  red[threadIdx.x] = a;
  if (op == 0) tree_max(red); else tree_sum(red);
  if (threadIdx.x == 0) out[0] = red[0];
}

// psum[c] = sum over chunk c of exp(logp - M)
__global__ void __launch_bounds__(NT) k_sumexp(const double* __restrict__ logp, uint64_t Q, uint64_t nchunks,
                                               const double* __restrict__ M, double* __restrict__ psum) {
  __shared__ double red[NT];
  const double mx = M[0];
  for (uint64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    double a = 0.0;
    for (int k = 0; k < CH / NT; k++) {
      const uint64_t idx = c * CH + (uint64_t)k * NT + threadIdx.x;
      if (idx < Q) a += exp(logp[idx] - mx);
    }
    red[threadIdx.x] = a;
    tree_sum(red);
    if (threadIdx.x == 0) psum[c] = red[0];
    __syncthreads();
  }
}

__global__ void __launch_bounds__(NT) k_normalise(double* __restrict__ p, uint64_t Q, double logZ) {
  for (uint64_t idx = (uint64_t)blockIdx.x * NT + threadIdx.x; idx < Q; idx += (uint64_t)gridDim.x * NT)
    p[idx] = exp(p[idx] - logZ);
}

// The one strided reduction behind every marginal of the enumeration.  src is viewed as [A, Q1, M, Q2, B] (C order);
// bin (m1, m2) sums its complement (a, mm, b) - C = A M B elements, in pieces of CH: the threads of a workgroup take a
// piece strided and meet in the tree.  One piece: the result goes to dst[m1 os1 + m2 os2]; more: to part[bin][piece],
// which k_reduce_final sums.  shB / shM: log2 of B / M where they are powers of two (else -1).
__global__ void __launch_bounds__(NT) k_reduce(const double* __restrict__ src, uint64_t Q1, uint64_t M, uint64_t Q2, uint64_t B,
                                               int shB, int shM, uint64_t C, uint64_t npieces, uint64_t work,
                                               double* __restrict__ dst, int64_t os1, int64_t os2, double* __restrict__ part) {
  __shared__ double red[NT];
  for (uint64_t w = blockIdx.x; w < work; w += gridDim.x) {
    const uint64_t bin = w / npieces, piece = w - bin * npieces;
    const uint64_t m1 = bin / Q2, m2 = bin - m1 * Q2;
    const uint64_t c0 = piece * CH, c1 = c0 + CH < C ? c0 + CH : C;
    double acc = 0.0;
    for (uint64_t c = c0 + threadIdx.x; c < c1; c += NT) {
      uint64_t b, r, mm, a;
      if (shB >= 0) { b = c & (B - 1); r = c >> shB; } else { r = c / B; b = c - r * B; }
      if (shM >= 0) { mm = r & (M - 1); a = r >> shM; } else { a = r / M; mm = r - a * M; }
      acc += src[(((a * Q1 + m1) * M + mm) * Q2 + m2) * B + b];
    }
    red[threadIdx.x] = acc;
    tree_sum(red);
    if (threadIdx.x == 0) {
      if (npieces == 1) dst[(int64_t)m1 * os1 + (int64_t)m2 * os2] = red[0];
      else part[w] = red[0];
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(NT) k_reduce_final(const double* __restrict__ part, uint64_t bins, uint64_t npieces, uint64_t Q2,
                                                     double* __restrict__ dst, int64_t os1, int64_t os2) {
  __shared__ double red[NT];
  for (uint64_t bin = blockIdx.x; bin < bins; bin += gridDim.x) {
    double acc = 0.0;
    for (uint64_t k = threadIdx.x; k < npieces; k += NT) acc += part[bin * npieces + k];
    red[threadIdx.x] = acc;
    tree_sum(red);
    if (threadIdx.x == 0) {
      const uint64_t m1 = bin / Q2, m2 = bin - m1 * Q2;
      dst[(int64_t)m1 * os1 + (int64_t)m2 * os2] = red[0];
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------ method 1: global-state transfer
// col[i][s]: offset of the column (x_nbrs, x_i) of node i's dense table in the global state s (x' = 0)
__global__ void __launch_bounds__(NT) k_col(const Node* __restrict__ nodes, const int32_t* __restrict__ nbr_ptr,
                                            const int32_t* __restrict__ nbr, const int32_t* __restrict__ sstride, int N, int S,
                                            int q, int32_t* __restrict__ col) {
  const int64_t idx = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (idx >= (int64_t)N * S) return;
  const int i = (int)(idx / S), s = (int)(idx - (int64_t)i * S);
  int64_t c = 0;
  for (int p = nbr_ptr[i + 1] - 1; p >= nbr_ptr[i]; p--) { const int j = nbr[p]; c = c * q + (s / sstride[j]) % nodes[j].qi; }
  c = (c * q + (s / sstride[i]) % nodes[i].qi) * q;
  col[idx] = (int32_t)c;
}

// g_t(s) = prod_i phi_i^t(s_i) prod_{directed (j,i)} psi^{1/2}, from the tables of logarithms the enumeration uses
__global__ void __launch_bounds__(NT) k_g(const Node* __restrict__ nodes, const int32_t* __restrict__ nbr_ptr,
                                          const int32_t* __restrict__ nbr, const int32_t* __restrict__ in_edge,
                                          const int32_t* __restrict__ sstride, const double* __restrict__ logphi,
                                          const double* __restrict__ hlpsi, int N, int L, int S, int q, double* __restrict__ g) {
  const int64_t idx = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (idx >= (int64_t)L * S) return;
  const int t = (int)(idx / S), s = (int)(idx - (int64_t)t * S);
  double acc = 0.0;
  for (int i = 0; i < N; i++) {
    const int x = (s / sstride[i]) % nodes[i].qi;
    acc += logphi[((size_t)i * L + t) * q + x];
    for (int p = nbr_ptr[i]; p < nbr_ptr[i + 1]; p++) {
      const int j = nbr[p];
      acc += hlpsi[(((size_t)in_edge[p] * L + t) * q + x) * q + (s / sstride[j]) % nodes[j].qi];
    }
  }
  g[idx] = exp(acc);
}

// K[s, a] = prod_{i in [n0, n1)} W_i^t(a_i | s): the row-wise Kronecker product of the tables of one half of the nodes
__global__ void __launch_bounds__(NT) k_kron(const Node* __restrict__ nodes, const double* __restrict__ w,
                                             const int32_t* __restrict__ col, int n0, int n1, int S, int SX, int t,
                                             double* __restrict__ K) {
  const int64_t idx = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (idx >= (int64_t)S * SX) return;
  const int s = (int)(idx / SX);
  int r = (int)(idx - (int64_t)s * SX);
  double prod = 1.0;
  for (int i = n1 - 1; i >= n0; i--) {
    const Node nd = nodes[i];
    const int nr = r / nd.qi, x = r - nr * nd.qi;
    r = nr;
    prod *= w[nd.tab_base + (nd.nt > 1 ? (int64_t)t * nd.tstride : 0) + col[(int64_t)i * S + s] + x];
  }
  K[idx] = prod;
}

// forward product: part[chunk][A', B'] = sum over the chunk's states s (in order) of a(s) KA[s, A'] KB[s, B']
__global__ void __launch_bounds__(NT) k_fwd(const double* __restrict__ a, const double* __restrict__ KA,
                                            const double* __restrict__ KB, int S, int SA, int SB, int KC, int tilesB,
                                            double* __restrict__ part) {
  __shared__ double sA[KS][TS], sB[KS][TS];
  const int tA = blockIdx.x / tilesB, tB = blockIdx.x - tA * tilesB;
  const int A0 = tA * TS, B0 = tB * TS;
  const int s0 = blockIdx.y * KC, s1 = min(S, s0 + KC);
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  double acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) acc[i][j] = 0.0;
  for (int sb = s0; sb < s1; sb += KS) {
    for (int l = threadIdx.x; l < KS * TS; l += NT) {
      const int k = l / TS, c = l - k * TS, s = sb + k;
      double va = 0.0, vb = 0.0;
      if (s < s1) {
        if (A0 + c < SA) va = a[s] * KA[(size_t)s * SA + A0 + c];
        if (B0 + c < SB) vb = KB[(size_t)s * SB + B0 + c];
      }
      sA[k][c] = va; sB[k][c] = vb;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < KS; k++) {
      double ra[4], rb[4];
#pragma unroll
      for (int i = 0; i < 4; i++) { ra[i] = sA[k][ty * 4 + i]; rb[i] = sB[k][tx * 4 + i]; }
#pragma unroll
      for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[i][j] += ra[i] * rb[j];
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int A = A0 + ty * 4 + i, B = B0 + tx * 4 + j;
      if (A < SA && B < SB) part[(size_t)blockIdx.y * S + (size_t)A * SB + B] = acc[i][j];
    }
}

// backward product: part[B tile][s] = sum_{B in tile} KB[s, B] sum_A KA[s, A] H[A, B]
__global__ void __launch_bounds__(NT) k_bwd(const double* __restrict__ KA, const double* __restrict__ KB,
                                            const double* __restrict__ H, int S, int SA, int SB, double* __restrict__ part) {
  __shared__ double sK[KS][TS + 1], sH[KS][TS], red[TS][17];
  const int s0 = blockIdx.x * TS, B0 = blockIdx.y * TS;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  double acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) acc[i][j] = 0.0;
  for (int A0 = 0; A0 < SA; A0 += KS) {
    for (int l = threadIdx.x; l < KS * TS; l += NT) {
      const int r = l / KS, k = l - r * KS, s = s0 + r, A = A0 + k;
      sK[k][r] = (s < S && A < SA) ? KA[(size_t)s * SA + A] : 0.0;
    }
    for (int l = threadIdx.x; l < KS * TS; l += NT) {
      const int k = l / TS, c = l - k * TS, A = A0 + k, B = B0 + c;
      sH[k][c] = (A < SA && B < SB) ? H[(size_t)A * SB + B] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < KS; k++) {
      double ra[4], rb[4];
#pragma unroll
      for (int i = 0; i < 4; i++) { ra[i] = sK[k][ty * 4 + i]; rb[i] = sH[k][tx * 4 + i]; }
#pragma unroll
      for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[i][j] += ra[i] * rb[j];
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int s = s0 + ty * 4 + i;
    double r = 0.0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int B = B0 + tx * 4 + j;
      if (s < S && B < SB) r += acc[i][j] * KB[(size_t)s * SB + B];
    }
    red[ty * 4 + i][tx] = r;
  }
  __syncthreads();
  if (threadIdx.x < TS) {
    const int s = s0 + threadIdx.x;
    double r = 0.0;
    for (int k = 0; k < 16; k++) r += red[threadIdx.x][k];
    if (s < S) part[(size_t)blockIdx.y * S + s] = r;
  }
}

// out[s] = (mul ? mul[s] : 1) * sum_k part[k][s], the partials in order
__global__ void __launch_bounds__(NT) k_gather(const double* __restrict__ part, int nparts, int S, const double* __restrict__ mul,
                                               double* __restrict__ out) {
  const int s = blockIdx.x * NT + threadIdx.x;
  if (s >= S) return;
  double v = 0.0;
  for (int k = 0; k < nparts; k++) v += part[(size_t)k * S + s];
  out[s] = mul ? mul[s] * v : v;
}

// one workgroup: z = sum v (fixed order), v /= z, zout = z; then out1 = mul1 * v and inout2 *= v where given
__global__ void __launch_bounds__(NT) k_scale(double* __restrict__ v, int S, double* __restrict__ zout, const double* __restrict__ mul1,
                                              double* __restrict__ out1, double* __restrict__ inout2) {
  __shared__ double red[NT];
  double a = 0.0;
  for (int s = threadIdx.x; s < S; s += NT) a += v[s];
  red[threadIdx.x] = a;
  tree_sum(red);
  const double z = red[0];
  if (threadIdx.x == 0 && zout) zout[0] = z;
  for (int s = threadIdx.x; s < S; s += NT) {
    const double x = v[s] / z;
    v[s] = x;
    if (out1) out1[s] = mul1[s] * x;
    if (inout2) inout2[s] *= x;
  }
}

// node marginals of gamma_t: one workgroup per (t, i), out[x + q (t + L i)]
__global__ void __launch_bounds__(NT) k_tr_node(const double* __restrict__ gamma, const Node* __restrict__ nodes,
                                                const int32_t* __restrict__ sstride, int N, int L, int S, int q,
                                                double* __restrict__ out) {
  __shared__ double red[NT];
  __shared__ double bins[MAXQ];
  const int t = blockIdx.x / N, i = blockIdx.x - t * N;
  const int qi = nodes[i].qi, st = sstride[i];
  double a[MAXQ] = {0.0, 0.0, 0.0, 0.0};
  for (int s = threadIdx.x; s < S; s += NT) {
    const double w = gamma[(size_t)t * S + s];
    const int x = (s / st) % qi;
#pragma unroll
    for (int k = 0; k < MAXQ; k++) a[k] += k == x ? w : 0.0;
  }
#pragma unroll
  for (int k = 0; k < MAXQ; k++) {
    red[threadIdx.x] = a[k];
    tree_sum(red);
    if (threadIdx.x == 0) bins[k] = red[0];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    double tot = 0.0;
    for (int k = 0; k < qi; k++) tot += bins[k];
    for (int k = 0; k < q; k++) out[k + (size_t)q * (t + (size_t)L * i)] = k < qi ? bins[k] / tot : 0.0;
  }
}

// same-time pair marginals of gamma_t: one workgroup per (t, e), out[x_src + q (x_dst + q (t + L e))]
__global__ void __launch_bounds__(NT) k_tr_pair(const double* __restrict__ gamma, const Node* __restrict__ nodes,
                                                const int32_t* __restrict__ sstride, const int32_t* __restrict__ esrc,
                                                const int32_t* __restrict__ edst, int E, int L, int S, int q,
                                                double* __restrict__ out) {
  __shared__ double red[NT];
  __shared__ double bins[MAXQ * MAXQ];
  const int t = blockIdx.x / E, e = blockIdx.x - t * E;
  const int i = esrc[e], j = edst[e];
  const int qi = nodes[i].qi, qj = nodes[j].qi, si = sstride[i], sj = sstride[j];
  double a[MAXQ * MAXQ];
#pragma unroll
  for (int k = 0; k < MAXQ * MAXQ; k++) a[k] = 0.0;
  for (int s = threadIdx.x; s < S; s += NT) {
    const double w = gamma[(size_t)t * S + s];
    const int kk = (s / si) % qi + MAXQ * ((s / sj) % qj);
#pragma unroll
    for (int k = 0; k < MAXQ * MAXQ; k++) a[k] += k == kk ? w : 0.0;
  }
#pragma unroll
  for (int k = 0; k < MAXQ * MAXQ; k++) {
    red[threadIdx.x] = a[k];
    tree_sum(red);
    if (threadIdx.x == 0) bins[k] = red[0];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    double tot = 0.0;
    for (int y = 0; y < qj; y++)
      for (int x = 0; x < qi; x++) tot += bins[x + MAXQ * y];
    for (int y = 0; y < q; y++)
      for (int x = 0; x < q; x++)
        out[x + (size_t)q * (y + (size_t)q * (t + (size_t)L * e))] = (x < qi && y < qj) ? bins[x + MAXQ * y] / tot : 0.0;
  }
}

// ------------------------------------------------------------------------------------------ method 1: conditioned vectors
// Two-time and alternate marginals push R conditioned row vectors through K at once.  V and OUT are row-major [Rpad][S],
// Rpad a multiple of 16 with the padding rows exactly 0.
constexpr int TT_NRT = 8, TT_RB = 16 * TT_NRT;   // MFMA row tiles and rows of one row block
constexpr int TT_LDV = KS + 1;                   // LDS row stride of the V tile: odd, so loader writes and MFMA operand reads spread over the banks

typedef double d4 __attribute__((ext_vector_type(4)));

// OUT[r, (A', B')] = sum_s V[r, s] KA[s, A'] KB[s, B'] as an fp64 MFMA GEMM (M = Rpad, N = K = S).  A workgroup owns 64
// columns and up to TT_RB rows: the tile KA (.) KB of a k-step is formed once in LDS and serves every row tile, so the MFMA
// stream holds LDS reads and MFMAs only.  Each wave sums its 16 columns over s = 0, 1, ... in MFMA steps of 4: the order
// depends on S alone, and a row never sees the rows that travel with it.
__global__ void __launch_bounds__(NT) k_tt_step(const double* __restrict__ V, const double* __restrict__ KA,
                                                const double* __restrict__ KB, int S, int SA, int SB, int Rpad,
                                                double* __restrict__ OUT) {
  __shared__ double sV[TT_RB][TT_LDV], sK[KS][TS];
  const int n0 = blockIdx.x * TS, r0 = blockIdx.y * TT_RB;
  const int nrt = min(TT_NRT, (Rpad - r0) / 16);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, l15 = lane & 15;
  const int vk = threadIdx.x & 15, vr = threadIdx.x >> 4;     // loader of V: state s0 + vk of the rows r0 + 16 j + vr
  const int kc = threadIdx.x & 63, kk0 = threadIdx.x >> 6;    // loader of K: column n0 + kc of the states s0 + kk0 + 4 j
  const int n = n0 + kc;
  const bool ncol = n < S;
  const int cA = ncol ? n / SB : 0, cB = ncol ? n - cA * SB : 0;
  d4 acc[TT_NRT];
#pragma unroll
  for (int j = 0; j < TT_NRT; j++) acc[j] = d4{0.0, 0.0, 0.0, 0.0};
  double pv[TT_NRT], pa[KS / 4], pb[KS / 4];
  auto fetch = [&](int s0) {
#pragma unroll
    for (int j = 0; j < TT_NRT; j++)
      pv[j] = (j < nrt && s0 + vk < S) ? V[(size_t)(r0 + 16 * j + vr) * S + s0 + vk] : 0.0;
#pragma unroll
    for (int j = 0; j < KS / 4; j++) {
      const int s = s0 + kk0 + 4 * j;
      const bool ok = ncol && s < S;
      pa[j] = ok ? KA[(size_t)s * SA + cA] : 0.0;
      pb[j] = ok ? KB[(size_t)s * SB + cB] : 0.0;
    }
  };
  fetch(0);
  for (int s0 = 0; s0 < S; s0 += KS) {
#pragma unroll
    for (int j = 0; j < TT_NRT; j++) sV[16 * j + vr][vk] = pv[j];
#pragma unroll
    for (int j = 0; j < KS / 4; j++) sK[kk0 + 4 * j][kc] = pa[j] * pb[j];
    __syncthreads();
    if (s0 + KS < S) fetch(s0 + KS);        // the next tiles travel while this one is multiplied
#pragma unroll
    for (int k4 = 0; k4 < KS / 4; k4++) {
      const double b = sK[4 * k4 + g][wave * 16 + l15];
#pragma unroll
      for (int j = 0; j < TT_NRT; j++)
        if (j < nrt) acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(sV[16 * j + l15][4 * k4 + g], b, acc[j], 0, 0, 0);
    }
    __syncthreads();
  }
  const int col = n0 + wave * 16 + l15;
  if (col < S) {
#pragma unroll
    for (int j = 0; j < TT_NRT; j++)
      if (j < nrt) {
#pragma unroll
        for (int v = 0; v < 4; v++) OUT[(size_t)(r0 + 16 * j + g + 4 * v) * S + col] = acc[j][v];   // C: row g + 4 v, column l15
      }
  }
}

__global__ void __launch_bounds__(NT) k_tt_fill(double* __restrict__ v, int S, double val) {
  const int s = blockIdx.x * NT + threadIdx.x;
  if (s < S) v[s] = val;
}

// admits an origin: the rows of member m (blockIdx.y) in the slot that starts at row `slot0` become a (.) [s_i = x]
__global__ void __launch_bounds__(NT) k_tt_admit(const double* __restrict__ a, const Node* __restrict__ nodes,
                                                 const int32_t* __restrict__ sstride, const int32_t* __restrict__ mem_row,
                                                 const int32_t* __restrict__ mem_node, int slot0, int S, double* __restrict__ V) {
  const int s = blockIdx.x * NT + threadIdx.x;
  if (s >= S) return;
  const int i = mem_node[blockIdx.y], qi = nodes[i].qi, xs = (s / sstride[i]) % qi;
  const double w = a[s];
  for (int x = 0; x < qi; x++) V[(size_t)(slot0 + mem_row[blockIdx.y] + x) * S + s] = x == xs ? w : 0.0;
}

// one workgroup per (member, slot): the q_i rows of the group are multiplied by g and divided by their common total
// (fixed order; a group that is identically zero stays zero)
__global__ void __launch_bounds__(NT) k_tt_scale(double* __restrict__ V, const double* __restrict__ gmul,
                                                 const Node* __restrict__ nodes, const int32_t* __restrict__ mem_row,
                                                 const int32_t* __restrict__ mem_node, int G, int S) {
  __shared__ double red[NT];
  const int qi = nodes[mem_node[blockIdx.x]].qi;
  double* v = V + (size_t)(blockIdx.y * G + mem_row[blockIdx.x]) * S;
  double a = 0.0;
  for (int x = 0; x < qi; x++)
    for (int s = threadIdx.x; s < S; s += NT) {
      const double w = v[(size_t)x * S + s] * gmul[s];
      v[(size_t)x * S + s] = w;
      a += w;
    }
  red[threadIdx.x] = a;
  tree_sum(red);
  const double z = red[0];
  if (!(z > 0.0)) return;
  for (int x = 0; x < qi; x++)
    for (int s = threadIdx.x; s < S; s += NT) v[(size_t)x * S + s] /= z;
}

// read-out after the step u -> u + 1: one workgroup per (read item, slot).  The slot holds the origin t, the latest one
// admitted into it; if it is still alive (t > u - md), bins[x][y] = sum_s v_x(s) b(s) [s_j = y] over the q_i rows of the
// item, divided by their total, go to out[base + t st_t + (u + 1) st_u + x + q y].  Padding entries stay as they are (0).
__global__ void __launch_bounds__(NT) k_tt_read(const double* __restrict__ V, const double* __restrict__ b,
                                                const Node* __restrict__ nodes, const int32_t* __restrict__ sstride,
                                                const int32_t* __restrict__ rd_row, const int32_t* __restrict__ rd_src,
                                                const int32_t* __restrict__ rd_dst, const int64_t* __restrict__ rd_base,
                                                int G, int W, int t1, int t2, int u, int md, int64_t st_t, int64_t st_u,
                                                int S, int q, double* __restrict__ out) {
  __shared__ double red[NT];
  __shared__ double bins[MAXQ * MAXQ];
  const int w = blockIdx.y, it = blockIdx.x;
  const int d = min(u, t2) - t1;
  const int t = t1 + d - (((d - w) % W) + W) % W;
  if (t < t1 || t + md <= u) return;
  const int qi = nodes[rd_src[it]].qi, j = rd_dst[it], qj = nodes[j].qi, sj = sstride[j];
  const double* v = V + (size_t)(w * G + rd_row[it]) * S;
  double a[MAXQ * MAXQ];
#pragma unroll
  for (int k = 0; k < MAXQ * MAXQ; k++) a[k] = 0.0;
  for (int s = threadIdx.x; s < S; s += NT) {
    const double bw = b[s];
    const int y = (s / sj) % qj;
#pragma unroll
    for (int x = 0; x < MAXQ; x++) {
      const double val = x < qi ? v[(size_t)x * S + s] * bw : 0.0;
#pragma unroll
      for (int yy = 0; yy < MAXQ; yy++) a[x + MAXQ * yy] += yy == y ? val : 0.0;
    }
  }
#pragma unroll
  for (int k = 0; k < MAXQ * MAXQ; k++) {
    red[threadIdx.x] = a[k];
    tree_sum(red);
    if (threadIdx.x == 0) bins[k] = red[0];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    double tot = 0.0;
    for (int y = 0; y < qj; y++)
      for (int x = 0; x < qi; x++) tot += bins[x + MAXQ * y];
    double* o = out + rd_base[it] + (int64_t)t * st_t + (int64_t)(u + 1) * st_u;
    for (int y = 0; y < qj; y++)
      for (int x = 0; x < qi; x++) o[x + q * y] = tot > 0.0 ? bins[x + MAXQ * y] / tot : 0.0;
  }
}

}  // namespace ex

// ================================================================================================ host side
struct mpbp_exact {
  mpbp_ctx* ctx = nullptr;
  int method = 0;
  uint64_t version = ~uint64_t(0);    // ctx->version the device tables were built from
  std::vector<int32_t> nbr;
  std::vector<uint64_t> Qn;           // q_i^(T+1)
  // tables (both methods)
  ex::Node* d_nodes = nullptr; double* d_tab = nullptr;
  int32_t *d_nbr_ptr = nullptr, *d_nbr = nullptr, *d_in_edge = nullptr, *d_esrc = nullptr, *d_edst = nullptr;
  double *d_logphi = nullptr, *d_hlpsi = nullptr;
  // enumeration
  uint64_t Q = 0, nchunks = 0;
  bool have_p = false, user_p = false;
  double* d_p = nullptr; double *d_pmax = nullptr, *d_psum = nullptr, *d_res = nullptr;
  double* d_part = nullptr; size_t part_cap = 0;
  double* d_site = nullptr; size_t site_cap = 0;
  double* d_edge = nullptr; size_t edge_cap = 0;
  double* d_out = nullptr; size_t out_cap = 0;
  // transfer
  int S = 0, SA = 1, SB = 1, nA = 0, KC = 256, nchunkS = 1, tilesA = 1, tilesB = 1;
  bool solved = false, one_block = false;
  int32_t *d_sstride = nullptr, *d_col = nullptr;
  double *d_g = nullptr, *d_a = nullptr, *d_b = nullptr, *d_H = nullptr, *d_KA = nullptr, *d_KB = nullptr, *d_tpart = nullptr,
         *d_z = nullptr;
  // conditioned vectors (two-time and alternate marginals): a_t and b_t of every t, kept from the first such call on
  double *d_aa = nullptr, *d_bb = nullptr;
  double* d_V[2] = {nullptr, nullptr}; size_t V_cap[2] = {0, 0};
  int32_t *d_mem_row = nullptr, *d_mem_node = nullptr, *d_rd_row = nullptr, *d_rd_src = nullptr, *d_rd_dst = nullptr;
  int64_t* d_rd_base = nullptr;
  double logZ = std::numeric_limits<double>::quiet_NaN();

  int fail(int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    ctx->err = buf; return code;
  }
};

#define XCHK(x, call)                                                                                     \
  do {                                                                                                    \
    hipError_t e_ = (call);                                                                               \
    if (e_ != hipSuccess) {                                                                               \
      (void)hipStreamSynchronize((x)->ctx->stream);                                                       \
      return (x)->fail(e_ == hipErrorOutOfMemory ? MPBP_ENOMEM : MPBP_EHIP, "%s failed: %s (%s:%d)", #call, \
                       hipGetErrorString(e_), __FILE__, __LINE__);                                        \
    }                                                                                                     \
  } while (0)

template <class T>
static hipError_t ex_upload(T*& dst, const std::vector<T>& v, hipStream_t st) {
  if (dst) { hipFree(dst); dst = nullptr; }
  hipError_t e = hipMalloc((void**)&dst, sizeof(T) * std::max<size_t>(v.size(), 1));
  if (e != hipSuccess) return e;
  if (v.empty()) return hipSuccess;
  e = hipMemcpyAsync(dst, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return e;
  return hipStreamSynchronize(st);
}

// grows a device buffer of doubles (contents are not preserved)
static hipError_t ex_reserve(double*& p, size_t& cap, size_t n) {
  if (cap >= n && p) return hipSuccess;
  if (p) { hipFree(p); p = nullptr; cap = 0; }
  hipError_t e = hipMalloc((void**)&p, sizeof(double) * std::max<size_t>(n, 1));
  if (e == hipSuccess) cap = n;
  return e;
}

static int ilog2_exact(uint64_t v) {      // log2 of a power of two, else -1
  if (v == 0 || (v & (v - 1))) return -1;
  int s = 0;
  while ((uint64_t(1) << s) != v) s++;
  return s;
}

// The dense table of one time block of a recursive factor: prob_y0, then one neighbour after the other through prob_xy and
// the (1, k-1) block of prob_yy, closed with prob_y - the order in which the sampler's draw kernel folds them.
static void fold_block(const NodeFactor& f, int q, int b, double* W) {
  const int deg = f.deg;
  const int ny1 = deg > 0 ? f.ny[1] : 1;
  const int64_t n0 = (int64_t)f.ny[0] * q, nxy = deg > 0 ? (int64_t)deg * f.ny[1] * q * q : 0, nyb = (int64_t)q * q * f.ny[deg];
  const double* py0 = f.prob_y0.data() + b * n0;
  const double* pxyb = f.prob_xy.data() + b * nxy;
  const double* pyyb = f.prob_yy.data() + b * f.yy_tblock;
  const double* py = f.prob_y.data() + b * nyb;
  int nymax = 1;
  for (int l = 0; l <= deg; l++) nymax = std::max(nymax, f.ny[l]);
  std::vector<double> P(nymax), Pn(nymax);
  std::vector<int> xk(deg + 1, 0);
  int64_t ncol = q;
  for (int k = 0; k < deg; k++) ncol *= q;
  for (int64_t col = 0; col < ncol; col++) {
    int64_t r = col;
    const int x = (int)(r % q); r /= q;
    for (int k = 1; k <= deg; k++) { xk[k] = (int)(r % q); r /= q; }
    int len = f.ny[0];
    for (int y = 0; y < len; y++) P[y] = py0[y + (int64_t)len * x];
    for (int k = 1; k <= deg; k++) {
      const double* pxy = pxyb + (int64_t)(k - 1) * ny1 * q * q + (int64_t)ny1 * (xk[k] + q * x);
      const int nyk = f.ny[k];
      const double* pyy = pyyb + f.yy_off[1 * (deg + 1) + (k - 1)];
      for (int y = 0; y < nyk; y++) {
        double acc = 0.0;
        for (int y2 = 0; y2 < len; y2++)
          for (int y1 = 0; y1 < ny1; y1++)
            acc += pyy[y + (int64_t)nyk * (y1 + (int64_t)ny1 * (y2 + (int64_t)len * x))] * pxy[y1] * P[y2];
        Pn[y] = acc;
      }
      std::swap(P, Pn);
      len = nyk;
    }
    for (int xx = 0; xx < q; xx++) {
      double p = 0.0;
      for (int y = 0; y < len; y++) p += P[y] * py[xx + q * (x + (int64_t)q * y)];
      W[col * q + xx] = p;
    }
  }
}

// device tables from the context's current factors, node states, phi and psi (once per change of the inputs)
static int ex_refresh(mpbp_exact* x) {
  mpbp_ctx* c = x->ctx;
  if (x->version == c->version) return MPBP_OK;
  const int N = c->N, q = c->q;
  std::vector<ex::Node> nodes(N);
  std::vector<double> tab;
  for (int i = 0; i < N; i++) {
    const NodeFactor& f = c->fac[i];
    if (!f.set) return x->fail(MPBP_EINVAL, "factor of node %d was never set (mpbp_set_factor / mpbp_set_generic_factor)", i);
    int64_t sz = (int64_t)q * q;
    for (int k = 0; k < f.deg; k++) {
      sz *= q;
      if (sz > ex::MAX_TABLE) return x->fail(MPBP_EUNSUPPORTED, "node %d: the dense transition table of degree %d exceeds %lld entries", i, f.deg, (long long)ex::MAX_TABLE);
    }
    ex::Node& nd = nodes[i];
    nd.deg = f.deg; nd.nt = f.nt; nd.qi = c->qnode[i]; nd.pad = 0;
    nd.tab_base = (int64_t)tab.size(); nd.tstride = sz;
    if (f.generic) {
      tab.insert(tab.end(), f.gen_w.begin(), f.gen_w.end());
    } else {
      tab.resize(tab.size() + (size_t)sz * f.nt);
      for (int b = 0; b < f.nt; b++) fold_block(f, q, b, tab.data() + nd.tab_base + (int64_t)b * sz);
    }
  }
  if (x->method == 0)
    for (double& v : tab) v = std::log(v);
  std::vector<double> lphi(c->phi.size()), lpsi(c->psi.size());
  for (size_t k = 0; k < lphi.size(); k++) lphi[k] = std::log(c->phi[k]);
  for (size_t k = 0; k < lpsi.size(); k++) lpsi[k] = 0.5 * std::log(c->psi[k]);
  hipStream_t st = c->stream;
  XCHK(x, ex_upload(x->d_nodes, nodes, st));
  XCHK(x, ex_upload(x->d_tab, tab, st));
  XCHK(x, ex_upload(x->d_logphi, lphi, st));
  XCHK(x, ex_upload(x->d_hlpsi, lpsi, st));
  x->one_block = true;
  for (int i = 0; i < N; i++) x->one_block = x->one_block && c->fac[i].nt == 1;
  x->version = c->version;
  x->solved = false;
  if (!x->user_p) x->have_p = false;
  return MPBP_OK;
}

extern "C" void mpbp_exact_destroy(mpbp_exact* x) {
  if (!x) return;
  hipSetDevice(x->ctx->device);
  hipStreamSynchronize(x->ctx->stream);
  for (void* p : {(void*)x->d_nodes, (void*)x->d_tab, (void*)x->d_nbr_ptr, (void*)x->d_nbr, (void*)x->d_in_edge, (void*)x->d_esrc,
                  (void*)x->d_edst, (void*)x->d_logphi, (void*)x->d_hlpsi, (void*)x->d_p, (void*)x->d_pmax, (void*)x->d_psum,
                  (void*)x->d_res, (void*)x->d_part, (void*)x->d_site, (void*)x->d_edge, (void*)x->d_out, (void*)x->d_sstride,
                  (void*)x->d_col, (void*)x->d_g, (void*)x->d_a, (void*)x->d_b, (void*)x->d_H, (void*)x->d_KA, (void*)x->d_KB,
                  (void*)x->d_tpart, (void*)x->d_z, (void*)x->d_aa, (void*)x->d_bb, (void*)x->d_V[0], (void*)x->d_V[1],
                  (void*)x->d_mem_row, (void*)x->d_mem_node, (void*)x->d_rd_row, (void*)x->d_rd_src, (void*)x->d_rd_dst,
                  (void*)x->d_rd_base})
    if (p) hipFree(p);
  delete x;
}

extern "C" int mpbp_exact_create(mpbp_exact** out, mpbp_ctx* c, int32_t method) {
  if (!out || !c) return MPBP_EINVAL;
  *out = nullptr;
  const int N = c->N, L = c->L, E = c->E, q = c->q;
  if (method != 0 && method != 1) return c->fail(MPBP_EINVAL, "exact solver: method must be 0 (joint enumeration) or 1 (global-state transfer), got %d", method);
  // an aliased graph (a node that is its own neighbour, the reference's InfiniteRegularGraph) has no joint distribution
  std::vector<int32_t> nbr(c->nnz());
  for (int i = 0; i < N; i++)
    for (int p = c->nbr_ptr[i]; p < c->nbr_ptr[i + 1]; p++) {
      nbr[p] = c->edge_src[c->in_edge[p]];
      if (nbr[p] < 0 || nbr[p] == i || c->edge_dst[c->in_edge[p]] != i)
        return c->fail(MPBP_EUNSUPPORTED, "node %d: position %d is not an edge to another node (aliased graph): the exact solver needs an explicit graph", i, p);
    }
  for (int e = 0; e < E; e++)
    if (c->edge_src[e] < 0 || c->edge_dst[e] < 0) return c->fail(MPBP_EUNSUPPORTED, "edge %d has no end node in the neighbour lists", e);
  if (q > ex::MAXQ) return c->fail(MPBP_EUNSUPPORTED, "the exact solver supports at most %d states per variable (q = %d)", ex::MAXQ, q);
  hipSetDevice(c->device);
  uint64_t Q = 1;
  int S = 1;
  std::vector<uint64_t> Qn(N, 1);
  size_t need = 0;
  if (method == 0) {
    if ((int64_t)N * L > ex::MAX_DIGITS)
      return c->fail(MPBP_EUNSUPPORTED, "joint enumeration: N (T+1) = %lld digits exceed the limit %d; method 1 (global-state transfer) has no limit on T", (long long)N * L, ex::MAX_DIGITS);
    for (int i = 0; i < N; i++)
      for (int t = 0; t < L; t++) {
        Qn[i] *= (uint64_t)c->qnode[i];
        Q *= (uint64_t)c->qnode[i];
        if (Q > ex::MAX_Q)
          return c->fail(MPBP_EUNSUPPORTED, "joint enumeration: more than 2^32 configurations (N = %d, T = %d); method 1 (global-state transfer) handles up to 2^16 global states at any T", N, c->T);
      }
    const uint64_t nch = (Q + ex::CH - 1) / ex::CH;
    need = sizeof(double) * ((size_t)Q + 2 * (size_t)nch + 2 * ((size_t)Q / ex::CH) + 64);
  } else {
    int64_t s = 1;
    for (int i = 0; i < N; i++) {
      s *= c->qnode[i];
      if (s > ex::MAX_S)
        return c->fail(MPBP_EUNSUPPORTED, "global-state transfer: more than 2^16 global states (N = %d)", N);
    }
    S = (int)s;
    if (c->periodic)
      return c->fail(MPBP_EUNSUPPORTED, "global-state transfer on chains periodic in time (the trace form) is not implemented: use method 0 (joint enumeration)");
  }
  mpbp_exact* x = new mpbp_exact();
  x->ctx = c; x->method = method; x->nbr = nbr; x->Q = Q; x->Qn = Qn; x->S = S;
  x->nchunks = (Q + ex::CH - 1) / ex::CH;
  if (method == 1) {
    // halves: nodes [0, nA) carry the high digits of s', nodes [nA, N) the low ones; the most balanced split
    int best = 0; int64_t bestv = S;
    int64_t sa = 1;
    for (int nA = 0; nA <= N; nA++) {
      const int64_t v = std::max<int64_t>(sa, S / sa);
      if (v < bestv) { bestv = v; best = nA; }
      if (nA < N) sa *= c->qnode[nA];
    }
    x->nA = best;
    x->SA = 1;
    for (int i = 0; i < best; i++) x->SA *= c->qnode[i];
    x->SB = S / x->SA;
    x->KC = std::max(256, S / 64);
    x->nchunkS = (S + x->KC - 1) / x->KC;
    x->tilesA = (x->SA + ex::TS - 1) / ex::TS;
    x->tilesB = (x->SB + ex::TS - 1) / ex::TS;
    need = sizeof(double) * ((size_t)S * (x->SA + x->SB) + (size_t)std::max(x->nchunkS, x->tilesB) * S + (size_t)(2 * L + 2) * S) +
           sizeof(int32_t) * (size_t)N * S;
  }
  size_t fre = 0, tot = 0;
  if (hipMemGetInfo(&fre, &tot) != hipSuccess) { delete x; return c->fail(MPBP_EHIP, "hipMemGetInfo failed"); }
  if (need + (size_t(64) << 20) > fre) {
    delete x;
    return c->fail(MPBP_ENOMEM, "exact solver: the working set of %zu MiB does not fit the %zu MiB of free device memory", need >> 20, fre >> 20);
  }
  hipStream_t st = c->stream;
  auto chk = [&](hipError_t e) -> int {
    if (e == hipSuccess) return MPBP_OK;
    return c->fail(e == hipErrorOutOfMemory ? MPBP_ENOMEM : MPBP_EHIP, "exact solver graph upload failed: %s", hipGetErrorString(e));
  };
  std::vector<int32_t> sstride(N, 1);
  for (int i = N - 2; i >= 0; i--) sstride[i] = method == 1 ? sstride[i + 1] * c->qnode[i + 1] : 1;
  int rc;
  if ((rc = chk(ex_upload(x->d_nbr_ptr, c->nbr_ptr, st))) || (rc = chk(ex_upload(x->d_nbr, x->nbr, st))) ||
      (rc = chk(ex_upload(x->d_in_edge, c->in_edge, st))) || (rc = chk(ex_upload(x->d_esrc, c->edge_src, st))) ||
      (rc = chk(ex_upload(x->d_edst, c->edge_dst, st))) || (rc = chk(ex_upload(x->d_sstride, sstride, st))) ||
      (rc = chk(hipMalloc((void**)&x->d_res, sizeof(double) * 4)))) {
    mpbp_exact_destroy(x);
    return rc;
  }
  *out = x;
  return MPBP_OK;
}

// ------------------------------------------------------------------------------------------ enumeration, host
static int enum_alloc(mpbp_exact* x) {
  if (x->d_p) return MPBP_OK;
  XCHK(x, hipMalloc((void**)&x->d_p, sizeof(double) * (size_t)x->Q));
  XCHK(x, hipMalloc((void**)&x->d_pmax, sizeof(double) * (size_t)x->nchunks));
  XCHK(x, hipMalloc((void**)&x->d_psum, sizeof(double) * (size_t)x->nchunks));
  XCHK(x, ex_reserve(x->d_part, x->part_cap, 2 * ((size_t)x->Q / ex::CH) + 64));
  return MPBP_OK;
}

static int enum_solve(mpbp_exact* x) {
  mpbp_ctx* c = x->ctx;
  int rc = enum_alloc(x);
  if (rc) return rc;
  hipStream_t st = c->stream;
  const unsigned grid = (unsigned)std::min<uint64_t>(x->nchunks, 1u << 20);
  x->have_p = false; x->user_p = false;
  hipLaunchKernelGGL(ex::k_logp, dim3(grid), dim3(ex::NT), 0, st, x->d_nodes, x->d_tab, x->d_nbr_ptr, x->d_nbr, x->d_in_edge,
                     x->d_logphi, x->d_hlpsi, c->N, c->L, c->q, c->periodic ? 1 : 0, x->Q, x->nchunks, x->d_p, x->d_pmax);
  XCHK(x, hipGetLastError());
  hipLaunchKernelGGL(ex::k_reduce1, dim3(1), dim3(ex::NT), 0, st, x->d_pmax, x->nchunks, 0, x->d_res);
  XCHK(x, hipGetLastError());
  hipLaunchKernelGGL(ex::k_sumexp, dim3(grid), dim3(ex::NT), 0, st, x->d_p, x->Q, x->nchunks, x->d_res, x->d_psum);
  XCHK(x, hipGetLastError());
  hipLaunchKernelGGL(ex::k_reduce1, dim3(1), dim3(ex::NT), 0, st, x->d_psum, x->nchunks, 1, x->d_res + 1);
  XCHK(x, hipGetLastError());
  double h[2];
  XCHK(x, hipMemcpyAsync(h, x->d_res, sizeof h, hipMemcpyDeviceToHost, st));
  XCHK(x, hipStreamSynchronize(st));
  if (!(h[0] > -std::numeric_limits<double>::infinity()) || !(h[1] > 0.0) || !std::isfinite(h[0]) || !std::isfinite(h[1]))
    return x->fail(MPBP_EINVAL, "exact solver: every configuration has zero weight (Z = 0): the observations exclude all trajectories");
  x->logZ = h[0] + std::log(h[1]);
  hipLaunchKernelGGL(ex::k_normalise, dim3((unsigned)std::min<uint64_t>((x->Q + ex::NT - 1) / ex::NT, 1u << 20)), dim3(ex::NT), 0, st,
                     x->d_p, x->Q, x->logZ);
  XCHK(x, hipGetLastError());
  XCHK(x, hipStreamSynchronize(st));
  x->have_p = true;
  return MPBP_OK;
}

// dst[m1 os1 + m2 os2] = sum over (a, mm, b) of src viewed as [A, Q1, M, Q2, B]
static int reduce5(mpbp_exact* x, const double* src, uint64_t A, uint64_t Q1, uint64_t M, uint64_t Q2, uint64_t B, double* dst,
                   int64_t os1, int64_t os2) {
  const uint64_t C = A * M * B, bins = Q1 * Q2, npieces = (C + ex::CH - 1) / ex::CH, work = bins * npieces;
  if (npieces > 1 && work > x->part_cap) XCHK(x, ex_reserve(x->d_part, x->part_cap, (size_t)work));
  hipStream_t st = x->ctx->stream;
  hipLaunchKernelGGL(ex::k_reduce, dim3((unsigned)std::min<uint64_t>(work, 1u << 20)), dim3(ex::NT), 0, st, src, Q1, M, Q2, B,
                     ilog2_exact(B), ilog2_exact(M), C, npieces, work, dst, os1, os2, x->d_part);
  XCHK(x, hipGetLastError());
  if (npieces > 1) {
    hipLaunchKernelGGL(ex::k_reduce_final, dim3((unsigned)std::min<uint64_t>(bins, 1u << 20)), dim3(ex::NT), 0, st, x->d_part, bins,
                       npieces, Q2, dst, os1, os2);
    XCHK(x, hipGetLastError());
  }
  return MPBP_OK;
}

static uint64_t prod_range(const std::vector<uint64_t>& v, int a, int b) {   // product of v[a..b)
  uint64_t r = 1;
  for (int k = a; k < b; k++) r *= v[k];
  return r;
}
static uint64_t ipow(uint64_t b, int e) { uint64_t r = 1; while (e-- > 0) r *= b; return r; }

// trajectory marginal of node i into dst[traj]
static int enum_site(mpbp_exact* x, int i, double* dst) {
  const int N = x->ctx->N;
  return reduce5(x, x->d_p, prod_range(x->Qn, 0, i), x->Qn[i], 1, 1, prod_range(x->Qn, i + 1, N), dst, 1, 0);
}
// joint of the trajectories of nodes lo < hi into dst[traj_lo os_lo + traj_hi os_hi]
static int enum_edge(mpbp_exact* x, int lo, int hi, double* dst, int64_t os_lo, int64_t os_hi) {
  const int N = x->ctx->N;
  return reduce5(x, x->d_p, prod_range(x->Qn, 0, lo), x->Qn[lo], prod_range(x->Qn, lo + 1, hi), x->Qn[hi],
                 prod_range(x->Qn, hi + 1, N), dst, os_lo, os_hi);
}

static int enum_ready(mpbp_exact* x) {
  hipSetDevice(x->ctx->device);
  if (x->user_p && x->have_p) return MPBP_OK;
  int rc = ex_refresh(x);
  if (rc) return rc;
  if (x->have_p) return MPBP_OK;
  return enum_solve(x);
}

static int enum_marginals(mpbp_exact* x, double* out) {
  mpbp_ctx* c = x->ctx;
  const int N = c->N, L = c->L, q = c->q;
  const size_t n = (size_t)q * L * N;
  XCHK(x, ex_reserve(x->d_out, x->out_cap, n));
  XCHK(x, hipMemsetAsync(x->d_out, 0, sizeof(double) * n, c->stream));
  for (int i = 0; i < N; i++) {
    XCHK(x, ex_reserve(x->d_site, x->site_cap, (size_t)x->Qn[i]));
    int rc = enum_site(x, i, x->d_site);
    if (rc) return rc;
    const uint64_t qi = (uint64_t)c->qnode[i];
    for (int t = 0; t < L; t++)
      if ((rc = reduce5(x, x->d_site, ipow(qi, t), qi, 1, 1, ipow(qi, L - 1 - t), x->d_out + ((size_t)i * L + t) * q, 1, 0))) return rc;
  }
  XCHK(x, hipMemcpyAsync(out, x->d_out, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
  XCHK(x, hipStreamSynchronize(c->stream));
  return MPBP_OK;
}

static int enum_pair_marginals(mpbp_exact* x, double* out) {
  mpbp_ctx* c = x->ctx;
  const int E = c->E, L = c->L, q = c->q;
  const size_t n = (size_t)q * q * L * E;
  XCHK(x, ex_reserve(x->d_out, x->out_cap, n));
  XCHK(x, hipMemsetAsync(x->d_out, 0, sizeof(double) * n, c->stream));
  std::vector<char> done(E, 0);
  for (int e = 0; e < E; e++) {
    if (done[e]) continue;
    const int lo = std::min(c->edge_src[e], c->edge_dst[e]), hi = std::max(c->edge_src[e], c->edge_dst[e]);
    XCHK(x, ex_reserve(x->d_edge, x->edge_cap, (size_t)(x->Qn[lo] * x->Qn[hi])));
    int rc = enum_edge(x, lo, hi, x->d_edge, (int64_t)x->Qn[hi], 1);       // p is read once per undirected edge
    if (rc) return rc;
    const uint64_t ql = (uint64_t)c->qnode[lo], qh = (uint64_t)c->qnode[hi];
    for (int e2 = e; e2 < E; e2++) {
      const int s2 = c->edge_src[e2], d2 = c->edge_dst[e2];
      if (done[e2] || std::min(s2, d2) != lo || std::max(s2, d2) != hi) continue;
      done[e2] = 1;
      for (int t = 0; t < L; t++)
        if ((rc = reduce5(x, x->d_edge, ipow(ql, t), ql, ipow(ql, L - 1 - t) * ipow(qh, t), qh, ipow(qh, L - 1 - t),
                          x->d_out + ((size_t)e2 * L + t) * q * q, s2 == lo ? 1 : q, s2 == lo ? q : 1))) return rc;
    }
  }
  XCHK(x, hipMemcpyAsync(out, x->d_out, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
  XCHK(x, hipStreamSynchronize(c->stream));
  return MPBP_OK;
}

// ------------------------------------------------------------------------------------------ transfer, host
static int tr_alloc(mpbp_exact* x) {
  if (x->d_KA) return MPBP_OK;
  mpbp_ctx* c = x->ctx;
  const size_t S = (size_t)x->S, L = (size_t)c->L;
  XCHK(x, hipMalloc((void**)&x->d_col, sizeof(int32_t) * (size_t)c->N * S));
  XCHK(x, hipMalloc((void**)&x->d_g, sizeof(double) * L * S));
  XCHK(x, hipMalloc((void**)&x->d_a, sizeof(double) * L * S));
  XCHK(x, hipMalloc((void**)&x->d_b, sizeof(double) * S));
  XCHK(x, hipMalloc((void**)&x->d_H, sizeof(double) * S));
  XCHK(x, hipMalloc((void**)&x->d_z, sizeof(double) * L));
  XCHK(x, hipMalloc((void**)&x->d_tpart, sizeof(double) * (size_t)std::max(x->nchunkS, x->tilesB) * S));
  XCHK(x, hipMalloc((void**)&x->d_KB, sizeof(double) * S * x->SB));
  XCHK(x, hipMalloc((void**)&x->d_KA, sizeof(double) * S * x->SA));
  return MPBP_OK;
}

static int tr_kron(mpbp_exact* x, int t) {
  mpbp_ctx* c = x->ctx;
  const int S = x->S;
  hipLaunchKernelGGL(ex::k_kron, dim3((unsigned)(((int64_t)S * x->SA + ex::NT - 1) / ex::NT)), dim3(ex::NT), 0, c->stream, x->d_nodes,
                     x->d_tab, x->d_col, 0, x->nA, S, x->SA, t, x->d_KA);
  XCHK(x, hipGetLastError());
  hipLaunchKernelGGL(ex::k_kron, dim3((unsigned)(((int64_t)S * x->SB + ex::NT - 1) / ex::NT)), dim3(ex::NT), 0, c->stream, x->d_nodes,
                     x->d_tab, x->d_col, x->nA, c->N, S, x->SB, t, x->d_KB);
  XCHK(x, hipGetLastError());
  return MPBP_OK;
}

static int tr_solve(mpbp_exact* x) {
  mpbp_ctx* c = x->ctx;
  int rc = tr_alloc(x);
  if (rc) return rc;
  const int N = c->N, L = c->L, T = c->T, q = c->q, S = x->S;
  hipStream_t st = c->stream;
  x->solved = false;
  hipLaunchKernelGGL(ex::k_col, dim3((unsigned)(((int64_t)N * S + ex::NT - 1) / ex::NT)), dim3(ex::NT), 0, st, x->d_nodes, x->d_nbr_ptr,
                     x->d_nbr, x->d_sstride, N, S, q, x->d_col);
  XCHK(x, hipGetLastError());
  hipLaunchKernelGGL(ex::k_g, dim3((unsigned)(((int64_t)L * S + ex::NT - 1) / ex::NT)), dim3(ex::NT), 0, st, x->d_nodes, x->d_nbr_ptr,
                     x->d_nbr, x->d_in_edge, x->d_sstride, x->d_logphi, x->d_hlpsi, N, L, S, q, x->d_g);
  XCHK(x, hipGetLastError());
  const unsigned gS = (unsigned)((S + ex::NT - 1) / ex::NT);
  // forward: a_0 = g_0, a_{t+1} = g_{t+1} (a_t K_t), each normalised; log Z = sum of the logs of the normalisers
  XCHK(x, hipMemcpyAsync(x->d_a, x->d_g, sizeof(double) * S, hipMemcpyDeviceToDevice, st));
  hipLaunchKernelGGL(ex::k_scale, dim3(1), dim3(ex::NT), 0, st, x->d_a, S, x->d_z, (const double*)nullptr, (double*)nullptr, (double*)nullptr);
  XCHK(x, hipGetLastError());
  for (int t = 0; t < T; t++) {
    if (t == 0 || !x->one_block) { if ((rc = tr_kron(x, t))) return rc; }
    hipLaunchKernelGGL(ex::k_fwd, dim3(x->tilesA * x->tilesB, x->nchunkS), dim3(ex::NT), 0, st, x->d_a + (size_t)t * S, x->d_KA, x->d_KB,
                       S, x->SA, x->SB, x->KC, x->tilesB, x->d_tpart);
    XCHK(x, hipGetLastError());
    double* an = x->d_a + (size_t)(t + 1) * S;
    hipLaunchKernelGGL(ex::k_gather, dim3(gS), dim3(ex::NT), 0, st, x->d_tpart, x->nchunkS, S, x->d_g + (size_t)(t + 1) * S, an);
    XCHK(x, hipGetLastError());
    hipLaunchKernelGGL(ex::k_scale, dim3(1), dim3(ex::NT), 0, st, an, S, x->d_z + t + 1, (const double*)nullptr, (double*)nullptr, (double*)nullptr);
    XCHK(x, hipGetLastError());
  }
  std::vector<double> z(L);
  XCHK(x, hipMemcpyAsync(z.data(), x->d_z, sizeof(double) * L, hipMemcpyDeviceToHost, st));
  XCHK(x, hipStreamSynchronize(st));
  double lz = 0.0;
  for (int t = 0; t < L; t++) {
    if (!(z[t] > 0.0) || !std::isfinite(z[t]))
      return x->fail(MPBP_EINVAL, "exact solver: every configuration has zero weight (Z = 0): no trajectory survives the observations up to time %d", t);
    lz += std::log(z[t]);
  }
  x->logZ = lz;
  if (x->d_aa) XCHK(x, hipMemcpyAsync(x->d_aa, x->d_a, sizeof(double) * (size_t)L * S, hipMemcpyDeviceToDevice, st));
  if (x->d_bb) {
    hipLaunchKernelGGL(ex::k_tt_fill, dim3(gS), dim3(ex::NT), 0, st, x->d_bb + (size_t)T * S, S, 1.0);
    XCHK(x, hipGetLastError());
  }
  // backward: b_T = 1, b_t = K_t (g_{t+1} b_{t+1}), each rescaled; a_t is overwritten by gamma_t = a_t b_t
  XCHK(x, hipMemcpyAsync(x->d_H, x->d_g + (size_t)T * S, sizeof(double) * S, hipMemcpyDeviceToDevice, st));
  for (int t = T - 1; t >= 0; t--) {
    if (!x->one_block) { if ((rc = tr_kron(x, t))) return rc; }
    hipLaunchKernelGGL(ex::k_bwd, dim3((S + ex::TS - 1) / ex::TS, x->tilesB), dim3(ex::NT), 0, st, x->d_KA, x->d_KB, x->d_H, S, x->SA,
                       x->SB, x->d_tpart);
    XCHK(x, hipGetLastError());
    hipLaunchKernelGGL(ex::k_gather, dim3(gS), dim3(ex::NT), 0, st, x->d_tpart, x->tilesB, S, (const double*)nullptr, x->d_b);
    XCHK(x, hipGetLastError());
    hipLaunchKernelGGL(ex::k_scale, dim3(1), dim3(ex::NT), 0, st, x->d_b, S, (double*)nullptr, x->d_g + (size_t)t * S, x->d_H,
                       x->d_a + (size_t)t * S);
    XCHK(x, hipGetLastError());
    if (x->d_bb) XCHK(x, hipMemcpyAsync(x->d_bb + (size_t)t * S, x->d_b, sizeof(double) * S, hipMemcpyDeviceToDevice, st));
  }
  XCHK(x, hipStreamSynchronize(st));
  x->solved = true;
  return MPBP_OK;
}

static int tr_ready(mpbp_exact* x) {
  hipSetDevice(x->ctx->device);
  int rc = ex_refresh(x);
  if (rc) return rc;
  if (x->solved) return MPBP_OK;
  return tr_solve(x);
}

// ------------------------------------------------------------------------------------------ C ABI
extern "C" int mpbp_exact_solve(mpbp_exact* x, double* logZ) {
  if (!x) return MPBP_EINVAL;
  hipSetDevice(x->ctx->device);
  int rc;
  if (x->method == 0) {
    if (x->user_p) { x->user_p = false; x->have_p = false; }      // a loaded p is replaced by the model's
    if ((rc = ex_refresh(x))) return rc;
    if (!x->have_p && (rc = enum_solve(x))) return rc;
  } else if ((rc = tr_ready(x))) {
    return rc;
  }
  if (logZ) *logZ = x->logZ;
  return MPBP_OK;
}

extern "C" int mpbp_exact_marginals(mpbp_exact* x, double* out) {
  if (!x || !out) return MPBP_EINVAL;
  int rc;
  if (x->method == 0) {
    if ((rc = enum_ready(x))) return rc;
    return enum_marginals(x, out);
  }
  if ((rc = tr_ready(x))) return rc;
  mpbp_ctx* c = x->ctx;
  const int N = c->N, L = c->L, q = c->q;
  const size_t n = (size_t)q * L * N;
  XCHK(x, ex_reserve(x->d_out, x->out_cap, n));
  hipLaunchKernelGGL(ex::k_tr_node, dim3(L * N), dim3(ex::NT), 0, c->stream, x->d_a, x->d_nodes, x->d_sstride, N, L, x->S, q, x->d_out);
  XCHK(x, hipGetLastError());
  XCHK(x, hipMemcpyAsync(out, x->d_out, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
  XCHK(x, hipStreamSynchronize(c->stream));
  return MPBP_OK;
}

extern "C" int mpbp_exact_pair_marginals(mpbp_exact* x, double* out) {
  if (!x || !out) return MPBP_EINVAL;
  int rc;
  if (x->method == 0) {
    if ((rc = enum_ready(x))) return rc;
    return enum_pair_marginals(x, out);
  }
  if ((rc = tr_ready(x))) return rc;
  mpbp_ctx* c = x->ctx;
  const int E = c->E, L = c->L, q = c->q;
  const size_t n = (size_t)q * q * L * E;
  if (n == 0) return MPBP_OK;
  XCHK(x, ex_reserve(x->d_out, x->out_cap, n));
  hipLaunchKernelGGL(ex::k_tr_pair, dim3(L * E), dim3(ex::NT), 0, c->stream, x->d_a, x->d_nodes, x->d_sstride, x->d_esrc, x->d_edst, E, L,
                     x->S, q, x->d_out);
  XCHK(x, hipGetLastError());
  XCHK(x, hipMemcpyAsync(out, x->d_out, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
  XCHK(x, hipStreamSynchronize(c->stream));
  return MPBP_OK;
}

static int enum_only(mpbp_exact* x, const char* what) {
  if (x->method == 0) return MPBP_OK;
  return x->fail(MPBP_EUNSUPPORTED, "%s needs the joint distribution: the global-state transfer solver keeps one time at a time - use method 0 (joint enumeration)", what);
}

extern "C" int mpbp_exact_prob(mpbp_exact* x, double* p) {
  if (!x || !p) return MPBP_EINVAL;
  int rc;
  if ((rc = enum_only(x, "mpbp_exact_prob")) || (rc = enum_ready(x))) return rc;
  XCHK(x, hipMemcpy(p, x->d_p, sizeof(double) * (size_t)x->Q, hipMemcpyDeviceToHost));
  return MPBP_OK;
}

extern "C" int mpbp_exact_set_prob(mpbp_exact* x, const double* p) {
  if (!x || !p) return MPBP_EINVAL;
  int rc;
  if ((rc = enum_only(x, "mpbp_exact_set_prob"))) return rc;
  hipSetDevice(x->ctx->device);
  if ((rc = enum_alloc(x))) return rc;
  XCHK(x, hipMemcpy(x->d_p, p, sizeof(double) * (size_t)x->Q, hipMemcpyHostToDevice));
  x->have_p = true; x->user_p = true;
  x->logZ = std::numeric_limits<double>::quiet_NaN();
  return MPBP_OK;
}

extern "C" int mpbp_exact_site_marginals(mpbp_exact* x, int32_t node, double* out) {
  if (!x || !out) return MPBP_EINVAL;
  int rc;
  if ((rc = enum_only(x, "mpbp_exact_site_marginals"))) return rc;
  if (node < 0 || node >= x->ctx->N) return x->fail(MPBP_EINVAL, "node %d out of range", node);
  if ((rc = enum_ready(x))) return rc;
  XCHK(x, ex_reserve(x->d_site, x->site_cap, (size_t)x->Qn[node]));
  if ((rc = enum_site(x, node, x->d_site))) return rc;
  XCHK(x, hipMemcpyAsync(out, x->d_site, sizeof(double) * (size_t)x->Qn[node], hipMemcpyDeviceToHost, x->ctx->stream));
  XCHK(x, hipStreamSynchronize(x->ctx->stream));
  return MPBP_OK;
}

extern "C" int mpbp_exact_edge_marginals(mpbp_exact* x, int32_t edge, double* out) {
  if (!x || !out) return MPBP_EINVAL;
  int rc;
  if ((rc = enum_only(x, "mpbp_exact_edge_marginals"))) return rc;
  mpbp_ctx* c = x->ctx;
  if (edge < 0 || edge >= c->E) return x->fail(MPBP_EINVAL, "edge %d out of range", edge);
  if ((rc = enum_ready(x))) return rc;
  const int i = c->edge_src[edge], j = c->edge_dst[edge], lo = std::min(i, j), hi = std::max(i, j);
  const size_t n = (size_t)(x->Qn[lo] * x->Qn[hi]);
  XCHK(x, ex_reserve(x->d_edge, x->edge_cap, n));
  // out[traj_i][traj_j] whichever of the two comes first in p
  if ((rc = enum_edge(x, lo, hi, x->d_edge, i == lo ? (int64_t)x->Qn[hi] : 1, i == lo ? 1 : (int64_t)x->Qn[lo]))) return rc;
  XCHK(x, hipMemcpyAsync(out, x->d_edge, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
  XCHK(x, hipStreamSynchronize(c->stream));
  return MPBP_OK;
}

// ------------------------------------------------------------------------------------------ conditioned vectors, host
// Two-time marginals p(x_i^t, x_i^u) and alternate marginals p(x_i^t, x_j^{t+1}) at any T.  An origin (t, i, x) is the row
// vector v_t = a_t (.) [s_i = x]; it is carried forward by v_{u+1} = g_{u+1} (.) (v_u K_u) and read against b_u, at node i
// itself (two-time) or at the neighbours one step later (alternate).  The q_i rows of one (t, i) form a group that is
// rescaled by its common total, so every table keeps its proportions.  The rows live in W slots of G rows, one slot per
// live origin time; the members (nodes) and origin times are cut into passes whose W G rows respect the row cap.  No row
// sees its companions, so the cut does not change a bit of the result.
static int tt_ready(mpbp_exact* x) {
  hipSetDevice(x->ctx->device);
  int rc = ex_refresh(x);
  if (rc) return rc;
  if (!x->d_aa || !x->d_bb) {
    const size_t bytes = sizeof(double) * (size_t)x->ctx->L * x->S;
    size_t fre = 0, tot = 0;
    XCHK(x, hipMemGetInfo(&fre, &tot));
    if (2 * bytes + (size_t(64) << 20) > fre)
      return x->fail(MPBP_ENOMEM, "exact solver: a_t and b_t of every time (%zu MiB) do not fit the %zu MiB of free device memory", (2 * bytes) >> 20, fre >> 20);
    if (!x->d_aa) XCHK(x, hipMalloc((void**)&x->d_aa, bytes));
    if (!x->d_bb) XCHK(x, hipMalloc((void**)&x->d_bb, bytes));
    x->solved = false;           // the next solve keeps them (same arithmetic, same log Z)
  }
  if (x->solved) return MPBP_OK;
  return tr_solve(x);
}

static int tt_row_cap() {
  const char* e = std::getenv("MPBP_EXACT_TT_ROWS");
  long v = e ? std::atol(e) : 0;
  if (v <= 0) v = 512;
  return (int)std::min<long>(std::max<long>(v, ex::MAXQ), 1 << 20);
}

struct TTRead { int32_t src, dst; int64_t base; };   // rows of member `src`, read at node `dst`, written from out + base

// one pass: the members mem[m0, m1) with their read items, origins t1 .. t2, lifetime md, W slots
static int tt_pass(mpbp_exact* x, const std::vector<int32_t>& mem_node, const std::vector<std::vector<TTRead>>& reads, int m0, int m1,
                   int t1, int t2, int md, int W, int64_t st_t, int64_t st_u, double* d_out) {
  mpbp_ctx* c = x->ctx;
  const int T = c->T, S = x->S, q = c->q;
  hipStream_t st = c->stream;
  std::vector<int32_t> mrow, mnode, rrow, rsrc, rdst;
  std::vector<int64_t> rbase;
  int G = 0;
  for (int m = m0; m < m1; m++) {
    mrow.push_back(G); mnode.push_back(mem_node[m]);
    for (const TTRead& r : reads[m]) { rrow.push_back(G); rsrc.push_back(r.src); rdst.push_back(r.dst); rbase.push_back(r.base); }
    G += c->qnode[mem_node[m]];
  }
  const int nmem = m1 - m0, nrd = (int)rrow.size();
  if (nrd == 0) return MPBP_OK;
  const int Rpad = (W * G + 15) / 16 * 16;
  const size_t nV = (size_t)Rpad * S;
  if (x->V_cap[0] < nV || x->V_cap[1] < nV) {
    size_t fre = 0, tot = 0;
    XCHK(x, hipMemGetInfo(&fre, &tot));
    if (2 * nV * sizeof(double) + (size_t(64) << 20) > fre + (x->V_cap[0] + x->V_cap[1]) * sizeof(double))
      return x->fail(MPBP_ENOMEM, "exact solver: a batch of %d conditioned vectors (2 x %zu MiB) does not fit the %zu MiB of free device memory; lower MPBP_EXACT_TT_ROWS", Rpad, (nV * sizeof(double)) >> 20, fre >> 20);
  }
  for (int k = 0; k < 2; k++) {
    XCHK(x, ex_reserve(x->d_V[k], x->V_cap[k], nV));
    XCHK(x, hipMemsetAsync(x->d_V[k], 0, sizeof(double) * nV, st));
  }
  XCHK(x, ex_upload(x->d_mem_row, mrow, st));
  XCHK(x, ex_upload(x->d_mem_node, mnode, st));
  XCHK(x, ex_upload(x->d_rd_row, rrow, st));
  XCHK(x, ex_upload(x->d_rd_src, rsrc, st));
  XCHK(x, ex_upload(x->d_rd_dst, rdst, st));
  XCHK(x, ex_upload(x->d_rd_base, rbase, st));
  const unsigned gS = (unsigned)((S + ex::NT - 1) / ex::NT);
  int cur = 0, rc;
  const int ulast = std::min(T - 1, t2 + md - 1);
  for (int u = t1; u <= ulast; u++) {
    if (!x->one_block && (rc = tr_kron(x, u))) return rc;
    if (u <= t2) {
      hipLaunchKernelGGL(ex::k_tt_admit, dim3(gS, nmem), dim3(ex::NT), 0, st, x->d_aa + (size_t)u * S, x->d_nodes, x->d_sstride,
                         x->d_mem_row, x->d_mem_node, ((u - t1) % W) * G, S, x->d_V[cur]);
      XCHK(x, hipGetLastError());
    }
    hipLaunchKernelGGL(ex::k_tt_step, dim3((S + ex::TS - 1) / ex::TS, (Rpad + ex::TT_RB - 1) / ex::TT_RB), dim3(ex::NT), 0, st, x->d_V[cur],
                       x->d_KA, x->d_KB, S, x->SA, x->SB, Rpad, x->d_V[cur ^ 1]);
    XCHK(x, hipGetLastError());
    cur ^= 1;
    hipLaunchKernelGGL(ex::k_tt_scale, dim3(nmem, W), dim3(ex::NT), 0, st, x->d_V[cur], x->d_g + (size_t)(u + 1) * S, x->d_nodes,
                       x->d_mem_row, x->d_mem_node, G, S);
    XCHK(x, hipGetLastError());
    hipLaunchKernelGGL(ex::k_tt_read, dim3(nrd, W), dim3(ex::NT), 0, st, x->d_V[cur], x->d_bb + (size_t)(u + 1) * S, x->d_nodes,
                       x->d_sstride, x->d_rd_row, x->d_rd_src, x->d_rd_dst, x->d_rd_base, G, W, t1, t2, u, md, st_t, st_u, S, q, d_out);
    XCHK(x, hipGetLastError());
  }
  return MPBP_OK;
}

// all passes of one call: members are cut where a slot would exceed the row cap, origin times where the live slots would
static int tt_run(mpbp_exact* x, const std::vector<int32_t>& mem_node, const std::vector<std::vector<TTRead>>& reads, int md,
                  int64_t st_t, int64_t st_u, double* d_out) {
  mpbp_ctx* c = x->ctx;
  const int T = c->T, cap = tt_row_cap(), nm = (int)mem_node.size();
  int rc;
  if (x->one_block && (rc = tr_kron(x, 0))) return rc;
  const int life = std::min(md, T);
  for (int m0 = 0; m0 < nm;) {
    int m1 = m0, G = 0;
    while (m1 < nm && (m1 == m0 || G + c->qnode[mem_node[m1]] <= cap)) G += c->qnode[mem_node[m1++]];
    const int W = std::min(life, std::max(1, cap / G));
    if (W == life) {
      if ((rc = tt_pass(x, mem_node, reads, m0, m1, 0, T - 1, md, W, st_t, st_u, d_out))) return rc;
    } else {
      for (int t1 = 0; t1 < T; t1 += W)
        if ((rc = tt_pass(x, mem_node, reads, m0, m1, t1, std::min(T - 1, t1 + W - 1), md, W, st_t, st_u, d_out))) return rc;
    }
    m0 = m1;
  }
  return MPBP_OK;
}

extern "C" int mpbp_exact_twovar_marginals(mpbp_exact* x, const int32_t* nodes, int32_t n_nodes, int32_t maxdist, double* out) {
  if (!x || !out || n_nodes < 0 || (n_nodes > 0 && !nodes)) return MPBP_EINVAL;
  mpbp_ctx* c = x->ctx;
  const int N = c->N, L = c->L, T = c->T, q = c->q;
  for (int k = 0; k < n_nodes; k++)
    if (nodes[k] < 0 || nodes[k] >= N) return x->fail(MPBP_EINVAL, "mpbp_exact_twovar_marginals: node %d out of range", nodes[k]);
  const size_t n = (size_t)n_nodes * L * L * q * q;
  if (n == 0) return MPBP_OK;
  const int md = maxdist <= 0 ? std::max(T, 1) : std::min<int>(maxdist, std::max(T, 1));
  int rc;
  if ((rc = x->method == 0 ? enum_ready(x) : tt_ready(x))) return rc;
  XCHK(x, ex_reserve(x->d_out, x->out_cap, n));
  XCHK(x, hipMemsetAsync(x->d_out, 0, sizeof(double) * n, c->stream));
  const int64_t blk = (int64_t)q * q;
  if (x->method == 0) {
    // p viewed as [before, x_i^t, between, x_i^u, after]: one strided reduction per (k, t, u)
    for (int k = 0; k < n_nodes; k++) {
      const int i = nodes[k];
      const uint64_t qi = (uint64_t)c->qnode[i], pre = prod_range(x->Qn, 0, i), post = prod_range(x->Qn, i + 1, N);
      for (int t = 0; t < L; t++)
        for (int u = t + 1; u < L && u <= t + md; u++)
          if ((rc = reduce5(x, x->d_p, pre * ipow(qi, t), qi, ipow(qi, u - t - 1), qi, ipow(qi, L - 1 - u) * post,
                            x->d_out + (((int64_t)k * L + t) * L + u) * blk, 1, q))) return rc;
    }
  } else if (T > 0) {
    std::vector<int32_t> mem(nodes, nodes + n_nodes);
    std::vector<std::vector<TTRead>> reads(n_nodes);
    for (int k = 0; k < n_nodes; k++) reads[k].push_back(TTRead{nodes[k], nodes[k], (int64_t)k * L * L * blk});
    if ((rc = tt_run(x, mem, reads, md, (int64_t)L * blk, blk, x->d_out))) return rc;
  }
  XCHK(x, hipMemcpyAsync(out, x->d_out, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
  XCHK(x, hipStreamSynchronize(c->stream));
  return MPBP_OK;
}

extern "C" int mpbp_exact_alternate_marginals(mpbp_exact* x, double* out) {
  if (!x || !out) return MPBP_EINVAL;
  mpbp_ctx* c = x->ctx;
  const int N = c->N, L = c->L, T = c->T, E = c->E, q = c->q;
  const size_t n = (size_t)q * q * T * E;
  if (n == 0) return MPBP_OK;
  int rc;
  if ((rc = x->method == 0 ? enum_ready(x) : tt_ready(x))) return rc;
  XCHK(x, ex_reserve(x->d_out, x->out_cap, n));
  XCHK(x, hipMemsetAsync(x->d_out, 0, sizeof(double) * n, c->stream));
  const int64_t blk = (int64_t)q * q;
  if (x->method == 0) {
    // p viewed as [before, first kept digit, between, second kept digit, after]; the kept digits are (i, t) and (j, t + 1)
    for (int e = 0; e < E; e++) {
      const int i = c->edge_src[e], j = c->edge_dst[e], lo = std::min(i, j), hi = std::max(i, j);
      const uint64_t ql = (uint64_t)c->qnode[lo], qh = (uint64_t)c->qnode[hi];
      const uint64_t pre = prod_range(x->Qn, 0, lo), mid = prod_range(x->Qn, lo + 1, hi), post = prod_range(x->Qn, hi + 1, N);
      for (int t = 0; t < T; t++) {
        const int tl = i == lo ? t : t + 1, th = i == lo ? t + 1 : t;      // times kept at the lower and at the higher node
        if ((rc = reduce5(x, x->d_p, pre * ipow(ql, tl), ql, ipow(ql, L - 1 - tl) * mid * ipow(qh, th), qh, ipow(qh, L - 1 - th) * post,
                          x->d_out + ((int64_t)e * T + t) * blk, i == lo ? 1 : q, i == lo ? q : 1))) return rc;
      }
    }
  } else {
    std::vector<int32_t> mem;
    std::vector<std::vector<TTRead>> reads;
    for (int i = 0; i < N; i++) {
      std::vector<TTRead> r;
      for (int e = 0; e < E; e++)
        if (c->edge_src[e] == i) r.push_back(TTRead{i, c->edge_dst[e], (int64_t)e * T * blk});
      if (!r.empty()) { mem.push_back(i); reads.push_back(r); }
    }
    if ((rc = tt_run(x, mem, reads, 1, blk, 0, x->d_out))) return rc;
  }
  XCHK(x, hipMemcpyAsync(out, x->d_out, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
  XCHK(x, hipStreamSynchronize(c->stream));
  return MPBP_OK;
}
