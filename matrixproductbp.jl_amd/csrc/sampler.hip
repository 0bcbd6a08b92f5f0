// SoftMargin importance sampler (reference src/sampling.jl): trajectories drawn from the prior dynamics of a context's
// factors, weighted by the observations phi^{t>=1} and the pair potentials psi, accumulated on the device into node,
// pair and two-time marginals.  C ABI: mpbp_sampler_* in include/mpbp_hip.h.
//
// Every draw is a deterministic function of (seed, global sample index, t, node): one Philox4x32-10 block per
// (sample, time, node), so trajectories do not depend on the launch geometry or on how the caller splits its calls.
// Factor evaluation runs in fp64 in the reference's order with contraction off, so that a host restatement of the
// same arithmetic reproduces every draw (tests/test_sampling.py).
#pragma clang fp contract(off)

#include "ctx.h"

#include <cmath>
#include <limits>

namespace smp {

constexpr int MAXQ = 4;        // states per variable (mpbp_create accepts q <= 4)
constexpr int MAXNY = 64;      // states of the auxiliary variable y of a recursive factor
constexpr int NT = 256;        // threads per workgroup of every sampler kernel
constexpr int LDS_BUDGET = 32768;   // bytes of x^t / x^{t+1} per draw workgroup (S samples x N nodes x 2)
constexpr size_t X_BATCH_BYTES = size_t(256) << 20;   // device trajectories of one batch

struct Node {
  int32_t kind;      // 0 recursive, 1 generic
  int32_t deg, nt, qi;
  int32_t ny_base;   // ny[0..deg] at ny_base
  int32_t off_base;  // recursive: [o_xy, o_y, o_yy(k=1..deg)] at off_base (int64, relative to the time block)
  int64_t tab_base, tstride;
};

struct State {      // running accumulation state (device)
  double M;         // running maximum of log w
  double sw, sw2;   // sum of exp(log w - M), of exp(2 (log w - M))
  double scale;     // factor applied to the accumulators by the current batch: exp(M_old - M_new)
};

// ---------------------------------------------------------------------------------------------- Philox4x32-10
__host__ __device__ inline void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
  for (int r = 0; r < 10; r++) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0, hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
    const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
    c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
}

// the one uniform of (sample, t, node): 53 random bits from the first two words
__device__ inline double uniform(uint64_t seed, uint64_t sample, int t, int node) {
  uint32_t c[4] = {(uint32_t)sample, (uint32_t)(sample >> 32), (uint32_t)t, (uint32_t)node};
  philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  return ((double)(c[0] >> 5) * 67108864.0 + (double)(c[1] >> 6)) * (1.0 / 9007199254740992.0);
}

// ---------------------------------------------------------------------------------------------- kernels
// One workgroup per S consecutive samples of the batch; x^t and x^{t+1} of those samples live in LDS as uint8.
// MY bounds nstates(w, l) of the recursive factors: with MY = 4 (SIS, SIRS, small Glauber nodes) the fold loops unroll
// and the two vectors stay in registers; MY = MAXNY keeps them in scratch.  Skipped iterations add nothing, so the order
// of the additions - and every draw - is the same in both forms.
template <int MY>
__global__ void __launch_bounds__(NT) k_draw(const Node* __restrict__ nodes, const double* __restrict__ tab,
                                             const int32_t* __restrict__ nyv, const int64_t* __restrict__ offv,
                                             const int32_t* __restrict__ nbr_ptr, const int32_t* __restrict__ nbr,
                                             const double* __restrict__ p0, int N, int L, int q, int S, int nb,
                                             uint64_t first, uint64_t seed, uint8_t* __restrict__ X) {
  extern __shared__ uint8_t lds[];
  uint8_t* cur = lds;
  uint8_t* nxt = lds + (size_t)S * N;
  const int s0 = blockIdx.x * S;
  const int ns = min(S, nb - s0);
  const int total = ns * N;
  // x^0 ~ phi^0 / sum(phi^0): phi^0 does not enter the weight
  for (int idx = threadIdx.x; idx < total; idx += NT) {
    const int s = idx / N, i = idx - s * N;
    const double u = uniform(seed, first + s0 + s, 0, i);
    const int qi = nodes[i].qi;
    double cw = 0.0;
    int x = -1, lastnz = 0;
    for (int xx = 0; xx < qi; xx++) {
      const double p = p0[(size_t)i * q + xx];
      if (p > 0.0) lastnz = xx;
      cw += p;
      if (cw > u) { x = xx; break; }
    }
    if (x < 0) x = lastnz;
    cur[idx] = (uint8_t)x;
    X[((size_t)(s0 + s) * L) * N + i] = (uint8_t)x;
  }
  __syncthreads();
  constexpr int UNR = MY <= 8 ? MY : 1;
  double P[MY], Pn[MY];
  for (int t = 0; t + 1 < L; t++) {
    for (int idx = threadIdx.x; idx < total; idx += NT) {
      const int s = idx / N, i = idx - s * N;
      const uint8_t* xs = cur + (size_t)s * N;
      const Node nd = nodes[i];
      const int x = xs[i];
      const int pb = nbr_ptr[i];
      const double* tb = tab + nd.tab_base + (nd.nt > 1 ? (int64_t)t * nd.tstride : 0);
      const double u = uniform(seed, first + s0 + s, t + 1, i);
      double cw = 0.0;
      int xn = -1, lastnz = 0;
      if (nd.kind == 1) {
        // generic factor: w[x' + q (x + q (x_1 + q (x_2 + ...)))]
        int64_t col = 0;
        for (int k = nd.deg - 1; k >= 0; k--) col = col * q + xs[nbr[pb + k]];
        col = (col * q + x) * q;
        for (int xx = 0; xx < nd.qi; xx++) {
          const double p = tb[col + xx];
          if (p > 0.0) lastnz = xx;
          cw += p;
          if (cw > u) { xn = xx; break; }
        }
      } else {
        // the functor of a RecursiveBPFactor (reference src/recursive_bp_factor.jl:33-45)
        const int32_t* ny = nyv + nd.ny_base;
        const int64_t* of = offv + nd.off_base;
        const int ny1 = nd.deg > 0 ? ny[1] : 1;
        int len = ny[0];
#pragma unroll UNR
        for (int y = 0; y < MY; y++) P[y] = y < len ? tb[y + (int64_t)len * x] : 0.0;          // prob_y0
        for (int k = 1; k <= nd.deg; k++) {
          const int xk = xs[nbr[pb + k - 1]];
          const double* pxy = tb + of[0] + (int64_t)(k - 1) * ny1 * q * q + (int64_t)ny1 * (xk + q * x);
          const int nyk = ny[k];
          const double* pyy = tb + of[2 + k - 1];     // block (1, k-1): [y(ny[k])][y1(ny[1])][y2(ny[k-1])][x]
#pragma unroll UNR
          for (int y = 0; y < MY; y++) {
            double acc = 0.0;
            if (y < nyk) {
#pragma unroll UNR
              for (int y2 = 0; y2 < MY; y2++)
                if (y2 < len)
                  for (int y1 = 0; y1 < ny1; y1++)
                    acc += pyy[y + (int64_t)nyk * (y1 + (int64_t)ny1 * (y2 + (int64_t)len * x))] * pxy[y1] * P[y2];
            }
            Pn[y] = acc;
          }
#pragma unroll UNR
          for (int y = 0; y < MY; y++) P[y] = Pn[y];
          len = nyk;
        }
        const double* py = tb + of[1];                // prob_y [x'][x][y]
        for (int xx = 0; xx < nd.qi; xx++) {
          double p = 0.0;
#pragma unroll UNR
          for (int y = 0; y < MY; y++)
            if (y < len) p += P[y] * py[xx + q * (x + (int64_t)q * y)];
          if (p > 0.0) lastnz = xx;
          cw += p;
          if (cw > u) { xn = xx; break; }
        }
      }
      if (xn < 0) xn = lastnz;      // rounding left the running sum <= u (the reference asserts here)
      nxt[idx] = (uint8_t)xn;
      X[((size_t)(s0 + s) * L + t + 1) * N + i] = (uint8_t)xn;
    }
    __syncthreads();
    uint8_t* tmp = cur; cur = nxt; nxt = tmp;
  }
}

// log w of every sample of the batch: one workgroup per sample, a fixed-order tree over its threads
__global__ void __launch_bounds__(NT) k_logw(const uint8_t* __restrict__ X, const double* __restrict__ logphi,
                                             const double* __restrict__ hlpsi, const int32_t* __restrict__ nbr_ptr,
                                             const int32_t* __restrict__ nbr, const int32_t* __restrict__ in_edge,
                                             int N, int L, int q, double* __restrict__ lw) {
  __shared__ double red[NT];
  const size_t xs = (size_t)blockIdx.x * L * N;
  double acc = 0.0;
  for (int i = threadIdx.x; i < N; i += NT) {
    for (int t = 0; t < L; t++) {
      const uint8_t* xt = X + xs + (size_t)t * N;
      const int x = xt[i];
      if (t > 0) acc += logphi[((size_t)i * L + t) * q + x];
      for (int p = nbr_ptr[i]; p < nbr_ptr[i + 1]; p++)     // in-edge nbr -> i: psi[e][t][x_nbr][x_i]
        acc += hlpsi[(((size_t)in_edge[p] * L + t) * q + x) * q + xt[nbr[p]]];
    }
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int w = NT / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) lw[blockIdx.x] = red[0];
}

// one workgroup: running maximum, batch weights exp(log w - M), sums of w and w^2, the rescale of the accumulators
__global__ void __launch_bounds__(NT) k_weights(const double* __restrict__ lw, int nb, State* st, double* __restrict__ wb) {
  __shared__ double red[NT], red2[NT];
  const double ninf = -std::numeric_limits<double>::infinity();
  double m = ninf;
  for (int s = threadIdx.x; s < nb; s += NT) m = fmax(m, lw[s]);
  red[threadIdx.x] = m;
  __syncthreads();
  for (int w = NT / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + w]);
    __syncthreads();
  }
  const double Mold = st->M;
  const double Mnew = fmax(Mold, red[0]);
  __syncthreads();
  double a = 0.0, a2 = 0.0;
  for (int s = threadIdx.x; s < nb; s += NT) {
    const double w = Mnew == ninf ? 0.0 : exp(lw[s] - Mnew);
    wb[s] = w;
    a += w; a2 += w * w;
  }
  red[threadIdx.x] = a; red2[threadIdx.x] = a2;
  __syncthreads();
  for (int w = NT / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) { red[threadIdx.x] += red[threadIdx.x + w]; red2[threadIdx.x] += red2[threadIdx.x + w]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double sc = Mold == ninf ? 0.0 : exp(Mold - Mnew);     // accumulators are still zero while M = -inf
    st->sw = st->sw * sc + red[0];
    st->sw2 = st->sw2 * sc * sc + red2[0];
    st->M = Mnew;
    st->scale = sc;
  }
}

// node marginals: one thread per (t, i), acc[(x L + t) N + i]
__global__ void __launch_bounds__(NT) k_acc_node(const uint8_t* __restrict__ X, const double* __restrict__ wb, int nb,
                                                 int N, int L, int q, const State* st, double* __restrict__ acc) {
  const int idx = blockIdx.x * NT + threadIdx.x;
  if (idx >= N * L) return;
  double a[MAXQ] = {0.0, 0.0, 0.0, 0.0};
  for (int s = 0; s < nb; s++) {
    const double w = wb[s];
    const int x = X[(size_t)s * L * N + idx];
#pragma unroll
    for (int k = 0; k < MAXQ; k++) a[k] += k == x ? w : 0.0;
  }
  const double sc = st->scale;
  const size_t LN = (size_t)L * N;
#pragma unroll
  for (int k = 0; k < MAXQ; k++)
    if (k < q) acc[k * LN + idx] = acc[k * LN + idx] * sc + a[k];
}

// pair marginals: one thread per (t, e), acc[((x_src + q x_dst) L + t) E + e]
__global__ void __launch_bounds__(NT) k_acc_pair(const uint8_t* __restrict__ X, const double* __restrict__ wb, int nb,
                                                 int N, int L, int E, int q, const int32_t* __restrict__ esrc,
                                                 const int32_t* __restrict__ edst, const State* st, double* __restrict__ acc) {
  const int idx = blockIdx.x * NT + threadIdx.x;
  if (idx >= E * L) return;
  const int t = idx / E, e = idx - t * E;
  const int i = esrc[e], j = edst[e];
  double a[MAXQ * MAXQ];
#pragma unroll
  for (int k = 0; k < MAXQ * MAXQ; k++) a[k] = 0.0;
  for (int s = 0; s < nb; s++) {
    const double w = wb[s];
    const uint8_t* xt = X + ((size_t)s * L + t) * N;
    const int kk = xt[i] + q * xt[j];
#pragma unroll
    for (int k = 0; k < MAXQ * MAXQ; k++) a[k] += k == kk ? w : 0.0;
  }
  const double sc = st->scale;
  const size_t LE = (size_t)L * E;
#pragma unroll
  for (int k = 0; k < MAXQ * MAXQ; k++)
    if (k < q * q) acc[k * LE + idx] = acc[k * LE + idx] * sc + a[k];
}

// two-time joints of the requested sites: one thread per (site c, t, d = u - t in 1..D),
// acc[((x_t + q x_u) nc + c) L D + t D + d - 1]
__global__ void __launch_bounds__(NT) k_acc_corr(const uint8_t* __restrict__ X, const double* __restrict__ wb, int nb,
                                                 int N, int L, int q, const int32_t* __restrict__ sites, int nc, int D,
                                                 const State* st, double* __restrict__ acc) {
  const int idx = blockIdx.x * NT + threadIdx.x;
  if (idx >= nc * L * D) return;
  const int c = idx / (L * D), r = idx - c * L * D, t = r / D, u = t + 1 + (r - t * D);
  if (u >= L) return;
  const int i = sites[c];
  double a[MAXQ * MAXQ];
#pragma unroll
  for (int k = 0; k < MAXQ * MAXQ; k++) a[k] = 0.0;
  for (int s = 0; s < nb; s++) {
    const double w = wb[s];
    const uint8_t* xs = X + (size_t)s * L * N;
    const int kk = xs[(size_t)t * N + i] + q * xs[(size_t)u * N + i];
#pragma unroll
    for (int k = 0; k < MAXQ * MAXQ; k++) a[k] += k == kk ? w : 0.0;
  }
  const double sc = st->scale;
  const size_t n1 = (size_t)nc * L * D;
#pragma unroll
  for (int k = 0; k < MAXQ * MAXQ; k++)
    if (k < q * q) acc[k * n1 + idx] = acc[k * n1 + idx] * sc + a[k];
}

}  // namespace smp

// ================================================================================================ host side
struct mpbp_sampler {
  mpbp_ctx* ctx = nullptr;
  uint64_t seed = 0;
  int64_t count = 0;
  uint64_t version = ~uint64_t(0);    // ctx->version the device tables were built from
  int S = 1, B = 1;                   // samples per draw workgroup, per device batch
  int nymax = 1;                      // largest nstates(w, l) of the recursive factors (selects the draw kernel)
  std::vector<int32_t> sites; int D = 0;
  std::vector<int32_t> nbr, esrc, edst;
  std::string err;
  // device
  smp::Node* d_nodes = nullptr; double* d_tab = nullptr; int32_t* d_ny = nullptr; int64_t* d_off = nullptr;
  int32_t* d_nbr_ptr = nullptr; int32_t* d_nbr = nullptr; int32_t* d_in_edge = nullptr;
  int32_t* d_esrc = nullptr; int32_t* d_edst = nullptr; int32_t* d_sites = nullptr;
  double *d_p0 = nullptr, *d_logphi = nullptr, *d_hlpsi = nullptr;
  uint8_t* d_X = nullptr; double *d_lw = nullptr, *d_wb = nullptr;
  smp::State* d_st = nullptr;
  double *d_acc_node = nullptr, *d_acc_pair = nullptr, *d_acc_corr = nullptr;

  int fail(int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    err = buf; ctx->err = buf; return code;
  }
};

#define SCHK(s, call)                                                                                     \
  do {                                                                                                    \
    hipError_t e_ = (call);                                                                               \
    if (e_ != hipSuccess) {                                                                               \
      (void)hipStreamSynchronize((s)->ctx->stream);                                                       \
      return (s)->fail(e_ == hipErrorOutOfMemory ? MPBP_ENOMEM : MPBP_EHIP, "%s failed: %s (%s:%d)", #call, \
                       hipGetErrorString(e_), __FILE__, __LINE__);                                        \
    }                                                                                                     \
  } while (0)

template <class T>
static hipError_t upload(T*& dst, const std::vector<T>& v, hipStream_t st) {
  if (dst) { hipFree(dst); dst = nullptr; }
  hipError_t e = hipMalloc((void**)&dst, sizeof(T) * std::max<size_t>(v.size(), 1));
  if (e != hipSuccess) return e;
  if (v.empty()) return hipSuccess;
  e = hipMemcpyAsync(dst, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return e;
  return hipStreamSynchronize(st);
}

// device tables from the context's current factors, node states, phi and psi (once per change of the inputs)
static int refresh_tables(mpbp_sampler* s) {
  mpbp_ctx* c = s->ctx;
  if (s->version == c->version) return MPBP_OK;
  const int N = c->N, L = c->L, q = c->q;
  std::vector<smp::Node> nodes(N);
  std::vector<double> tab;
  std::vector<int32_t> ny;
  std::vector<int64_t> off;
  int nymax = 1;
  for (int i = 0; i < N; i++) {
    const NodeFactor& f = c->fac[i];
    if (!f.set) return s->fail(MPBP_EINVAL, "factor of node %d was never set (mpbp_set_factor / mpbp_set_generic_factor)", i);
    smp::Node& nd = nodes[i];
    nd.deg = f.deg; nd.nt = f.nt; nd.qi = c->qnode[i];
    nd.tab_base = (int64_t)tab.size();
    nd.ny_base = (int32_t)ny.size(); nd.off_base = (int32_t)off.size();
    if (f.generic) {
      nd.kind = 1;
      nd.tstride = (int64_t)(f.gen_w.size() / f.nt);
      tab.insert(tab.end(), f.gen_w.begin(), f.gen_w.end());
      continue;
    }
    nd.kind = 0;
    const int deg = f.deg;
    for (int l = 0; l <= deg; l++) {
      if (f.ny[l] > smp::MAXNY) return s->fail(MPBP_EUNSUPPORTED, "node %d: nstates(w, %d) = %d exceeds the sampler's limit %d", i, l, f.ny[l], smp::MAXNY);
      ny.push_back(f.ny[l]);
      nymax = std::max(nymax, f.ny[l]);
    }
    const int64_t n0 = (int64_t)f.ny[0] * q, nxy = deg > 0 ? (int64_t)deg * f.ny[1] * q * q : 0,
                  nyb = (int64_t)q * q * f.ny[deg];
    std::vector<int64_t> o_yy(deg);
    int64_t o = n0 + nxy;
    for (int k = 1; k <= deg; k++) { o_yy[k - 1] = o; o += (int64_t)f.ny[k] * f.ny[1] * f.ny[k - 1] * q; }
    const int64_t o_y = o;
    nd.tstride = o_y + nyb;
    off.push_back(n0); off.push_back(o_y);
    off.insert(off.end(), o_yy.begin(), o_yy.end());
    for (int b = 0; b < f.nt; b++) {
      tab.insert(tab.end(), f.prob_y0.begin() + b * n0, f.prob_y0.begin() + (b + 1) * n0);
      tab.insert(tab.end(), f.prob_xy.begin() + b * nxy, f.prob_xy.begin() + (b + 1) * nxy);
      for (int k = 1; k <= deg; k++) {
        const int64_t at = b * f.yy_tblock + f.yy_off[1 * (deg + 1) + (k - 1)];
        const int64_t n = (int64_t)f.ny[k] * f.ny[1] * f.ny[k - 1] * q;
        tab.insert(tab.end(), f.prob_yy.begin() + at, f.prob_yy.begin() + at + n);
      }
      tab.insert(tab.end(), f.prob_y.begin() + b * nyb, f.prob_y.begin() + (b + 1) * nyb);
    }
  }
  // p0_i = phi_i^0 / sum(phi_i^0); log phi; (1/2) log psi - in the ABI layouts of phi / psi
  std::vector<double> p0((size_t)N * q, 0.0), lphi(c->phi.size()), lpsi(c->psi.size());
  for (int i = 0; i < N; i++) {
    const double* ph = c->phi.data() + (size_t)q * L * i;
    double z = 0.0;
    for (int x = 0; x < c->qnode[i]; x++) z += ph[x];
    if (!(z > 0.0) || !std::isfinite(z)) return s->fail(MPBP_EINVAL, "node %d: phi at time 0 sums to %g; it must be a positive finite weight", i, z);
    for (int x = 0; x < c->qnode[i]; x++) p0[(size_t)i * q + x] = ph[x] / z;
  }
  for (size_t k = 0; k < lphi.size(); k++) lphi[k] = std::log(c->phi[k]);
  for (size_t k = 0; k < lpsi.size(); k++) lpsi[k] = 0.5 * std::log(c->psi[k]);
  hipStream_t st = c->stream;
  SCHK(s, upload(s->d_nodes, nodes, st));
  SCHK(s, upload(s->d_tab, tab, st));
  SCHK(s, upload(s->d_ny, ny, st));
  SCHK(s, upload(s->d_off, off, st));
  SCHK(s, upload(s->d_p0, p0, st));
  SCHK(s, upload(s->d_logphi, lphi, st));
  SCHK(s, upload(s->d_hlpsi, lpsi, st));
  s->nymax = nymax;
  s->version = c->version;
  return MPBP_OK;
}

extern "C" void mpbp_sampler_destroy(mpbp_sampler* s) {
  if (!s) return;
  hipSetDevice(s->ctx->device);
  hipStreamSynchronize(s->ctx->stream);
  for (void* p : {(void*)s->d_nodes, (void*)s->d_tab, (void*)s->d_ny, (void*)s->d_off, (void*)s->d_nbr_ptr, (void*)s->d_nbr,
                  (void*)s->d_in_edge, (void*)s->d_esrc, (void*)s->d_edst, (void*)s->d_sites, (void*)s->d_p0,
                  (void*)s->d_logphi, (void*)s->d_hlpsi, (void*)s->d_X, (void*)s->d_lw, (void*)s->d_wb, (void*)s->d_st,
                  (void*)s->d_acc_node, (void*)s->d_acc_pair, (void*)s->d_acc_corr})
    if (p) hipFree(p);
  delete s;
}

extern "C" int mpbp_sampler_create(mpbp_sampler** out, mpbp_ctx* c, uint64_t seed, const int32_t* corr_nodes,
                                   int32_t n_corr, int32_t maxdist) {
  if (!out || !c) return MPBP_EINVAL;
  *out = nullptr;
  const int N = c->N, L = c->L, E = c->E, q = c->q;
  if (q > smp::MAXQ) return c->fail(MPBP_EUNSUPPORTED, "the sampler supports at most %d states per variable (q = %d)", smp::MAXQ, q);
  if (n_corr < 0 || (n_corr > 0 && !corr_nodes)) return c->fail(MPBP_EINVAL, "corr_nodes: %d sites requested", n_corr);
  for (int k = 0; k < n_corr; k++)
    if (corr_nodes[k] < 0 || corr_nodes[k] >= N) return c->fail(MPBP_EINVAL, "corr_nodes[%d] = %d out of range", k, corr_nodes[k]);
  // neighbour of position p = source of its in-edge; an aliased graph (a node that is its own neighbour, the reference's
  // InfiniteRegularGraph) has no trajectory of its own
  std::vector<int32_t> nbr(c->nnz());
  for (int i = 0; i < N; i++)
    for (int p = c->nbr_ptr[i]; p < c->nbr_ptr[i + 1]; p++) {
      nbr[p] = c->edge_src[c->in_edge[p]];
      if (nbr[p] < 0 || nbr[p] == i || c->edge_dst[c->in_edge[p]] != i)
        return c->fail(MPBP_EUNSUPPORTED, "node %d: position %d is not an edge to another node (aliased graph): sampling needs an explicit graph", i, p);
    }
  for (int e = 0; e < E; e++)
    if (c->edge_src[e] < 0 || c->edge_dst[e] < 0) return c->fail(MPBP_EUNSUPPORTED, "edge %d has no end node in the neighbour lists", e);
  if (2 * N > 65536) return c->fail(MPBP_EUNSUPPORTED, "the sampler keeps two time steps of a sample in LDS: at most 32768 nodes (N = %d)", N);
  mpbp_sampler* s = new mpbp_sampler();
  s->ctx = c; s->seed = seed;
  s->nbr = nbr; s->esrc = c->edge_src; s->edst = c->edge_dst;
  s->sites.assign(corr_nodes, corr_nodes + n_corr);
  s->D = n_corr > 0 ? (maxdist >= 1 && maxdist <= c->T ? maxdist : c->T) : 0;
  {
    // batch: as many samples as X_BATCH_BYTES of trajectories hold; samples per workgroup: within the LDS budget, and
    // few enough that the batch spreads over >= 8 workgroups per CU (one sample per workgroup leaves most lanes idle
    // only on graphs far smaller than a workgroup, where the batch is then large)
    const int64_t per = (int64_t)L * N;
    int64_t B = std::max<int64_t>(1, (int64_t)(smp::X_BATCH_BYTES / per));
    B = std::min<int64_t>(B, 65536);
    const int64_t lds_cap = std::max(1, std::min(256, smp::LDS_BUDGET / (2 * N)));
    s->S = (int)std::max<int64_t>(1, std::min<int64_t>(lds_cap, B / (8 * (int64_t)c->num_cu)));
    s->B = (int)std::max<int64_t>(s->S, B / s->S * s->S);
  }
  hipSetDevice(c->device);
  hipStream_t st = c->stream;
  auto bail = [&](int rc) -> int { c->err = s->err; mpbp_sampler_destroy(s); return rc; };
  auto chk = [&](hipError_t e, const char* what) -> int {
    if (e == hipSuccess) return MPBP_OK;
    return s->fail(e == hipErrorOutOfMemory ? MPBP_ENOMEM : MPBP_EHIP, "%s failed: %s", what, hipGetErrorString(e));
  };
  int rc;
  if ((rc = chk(upload(s->d_nbr_ptr, c->nbr_ptr, st), "sampler graph upload")) ||
      (rc = chk(upload(s->d_nbr, s->nbr, st), "sampler graph upload")) ||
      (rc = chk(upload(s->d_in_edge, c->in_edge, st), "sampler graph upload")) ||
      (rc = chk(upload(s->d_esrc, s->esrc, st), "sampler graph upload")) ||
      (rc = chk(upload(s->d_edst, s->edst, st), "sampler graph upload")) ||
      (rc = chk(upload(s->d_sites, s->sites, st), "sampler sites upload")))
    return bail(rc);
  const size_t nn = (size_t)q * L * N, np = (size_t)q * q * L * E, ncr = (size_t)q * q * n_corr * L * std::max(s->D, 1);
  if ((rc = chk(hipMalloc((void**)&s->d_X, (size_t)s->B * L * N), "hipMalloc(sample batch)")) ||
      (rc = chk(hipMalloc((void**)&s->d_lw, sizeof(double) * s->B), "hipMalloc")) ||
      (rc = chk(hipMalloc((void**)&s->d_wb, sizeof(double) * s->B), "hipMalloc")) ||
      (rc = chk(hipMalloc((void**)&s->d_st, sizeof(smp::State)), "hipMalloc")) ||
      (rc = chk(hipMalloc((void**)&s->d_acc_node, sizeof(double) * nn), "hipMalloc(node accumulators)")) ||
      (rc = chk(hipMalloc((void**)&s->d_acc_pair, sizeof(double) * np), "hipMalloc(pair accumulators)")) ||
      (rc = chk(hipMalloc((void**)&s->d_acc_corr, sizeof(double) * std::max<size_t>(ncr, 1)), "hipMalloc(two-time accumulators)")))
    return bail(rc);
  smp::State h{-std::numeric_limits<double>::infinity(), 0.0, 0.0, 1.0};
  if ((rc = chk(hipMemcpy(s->d_st, &h, sizeof h, hipMemcpyHostToDevice), "hipMemcpy")) ||
      (rc = chk(hipMemset(s->d_acc_node, 0, sizeof(double) * nn), "hipMemset")) ||
      (rc = chk(hipMemset(s->d_acc_pair, 0, sizeof(double) * np), "hipMemset")) ||
      (rc = chk(hipMemset(s->d_acc_corr, 0, sizeof(double) * std::max<size_t>(ncr, 1)), "hipMemset")))
    return bail(rc);
  *out = s;
  return MPBP_OK;
}

extern "C" int mpbp_sample(mpbp_sampler* s, int64_t nsamples, uint8_t* X, double* logw) {
  if (!s) return MPBP_EINVAL;
  if (nsamples <= 0) return s->fail(MPBP_EINVAL, "nsamples must be positive (got %lld)", (long long)nsamples);
  mpbp_ctx* c = s->ctx;
  hipSetDevice(c->device);
  int rc = refresh_tables(s);
  if (rc != MPBP_OK) return rc;
  const int N = c->N, L = c->L, E = c->E, q = c->q;
  hipStream_t st = c->stream;
  const size_t lds = (size_t)2 * s->S * N;
  const int nc = (int)s->sites.size();
  for (int64_t done = 0; done < nsamples;) {
    const int nb = (int)std::min<int64_t>(s->B, nsamples - done);
    const uint64_t first = (uint64_t)(s->count + done);
    hipLaunchKernelGGL(s->nymax <= 4 ? smp::k_draw<4> : smp::k_draw<smp::MAXNY>, dim3((nb + s->S - 1) / s->S), dim3(smp::NT), lds, st, s->d_nodes, s->d_tab, s->d_ny,
                       s->d_off, s->d_nbr_ptr, s->d_nbr, s->d_p0, N, L, q, s->S, nb, first, s->seed, s->d_X);
    SCHK(s, hipGetLastError());
    hipLaunchKernelGGL(smp::k_logw, dim3(nb), dim3(smp::NT), 0, st, s->d_X, s->d_logphi, s->d_hlpsi, s->d_nbr_ptr, s->d_nbr,
                       s->d_in_edge, N, L, q, s->d_lw);
    SCHK(s, hipGetLastError());
    hipLaunchKernelGGL(smp::k_weights, dim3(1), dim3(smp::NT), 0, st, s->d_lw, nb, s->d_st, s->d_wb);
    SCHK(s, hipGetLastError());
    hipLaunchKernelGGL(smp::k_acc_node, dim3((N * L + smp::NT - 1) / smp::NT), dim3(smp::NT), 0, st, s->d_X, s->d_wb, nb,
                       N, L, q, s->d_st, s->d_acc_node);
    SCHK(s, hipGetLastError());
    hipLaunchKernelGGL(smp::k_acc_pair, dim3((E * L + smp::NT - 1) / smp::NT), dim3(smp::NT), 0, st, s->d_X, s->d_wb, nb,
                       N, L, E, q, s->d_esrc, s->d_edst, s->d_st, s->d_acc_pair);
    SCHK(s, hipGetLastError());
    if (nc > 0) {
      hipLaunchKernelGGL(smp::k_acc_corr, dim3((nc * L * s->D + smp::NT - 1) / smp::NT), dim3(smp::NT), 0, st, s->d_X,
                         s->d_wb, nb, N, L, q, s->d_sites, nc, s->D, s->d_st, s->d_acc_corr);
      SCHK(s, hipGetLastError());
    }
    if (X) SCHK(s, hipMemcpyAsync(X + (size_t)done * L * N, s->d_X, (size_t)nb * L * N, hipMemcpyDeviceToHost, st));
    if (logw) SCHK(s, hipMemcpyAsync(logw + done, s->d_lw, sizeof(double) * nb, hipMemcpyDeviceToHost, st));
    SCHK(s, hipStreamSynchronize(st));     // the batch buffer is reused by the next batch
    done += nb;
  }
  s->count += nsamples;
  return MPBP_OK;
}

static int read_state(mpbp_sampler* s, smp::State& h) {
  hipSetDevice(s->ctx->device);
  SCHK(s, hipMemcpy(&h, s->d_st, sizeof h, hipMemcpyDeviceToHost));
  return MPBP_OK;
}

static int normaliser(mpbp_sampler* s, double& sw) {
  if (s->count == 0) return s->fail(MPBP_EINVAL, "no samples drawn yet");
  smp::State h;
  int rc = read_state(s, h);
  if (rc) return rc;
  if (!(h.sw > 0.0)) return s->fail(MPBP_EINVAL, "all %lld sampled weights are zero: the observations exclude every drawn trajectory", (long long)s->count);
  sw = h.sw;
  return MPBP_OK;
}

extern "C" int mpbp_sampler_marginals(mpbp_sampler* s, double* out) {
  if (!s || !out) return MPBP_EINVAL;
  double sw;
  int rc = normaliser(s, sw);
  if (rc) return rc;
  const mpbp_ctx* c = s->ctx;
  const int N = c->N, L = c->L, q = c->q;
  std::vector<double> h((size_t)q * L * N);
  SCHK(s, hipMemcpy(h.data(), s->d_acc_node, sizeof(double) * h.size(), hipMemcpyDeviceToHost));
  for (int i = 0; i < N; i++)
    for (int t = 0; t < L; t++)
      for (int x = 0; x < q; x++) out[x + (size_t)q * (t + (size_t)L * i)] = h[((size_t)x * L + t) * N + i] / sw;
  return MPBP_OK;
}

extern "C" int mpbp_sampler_pair_marginals(mpbp_sampler* s, double* out) {
  if (!s || !out) return MPBP_EINVAL;
  double sw;
  int rc = normaliser(s, sw);
  if (rc) return rc;
  const mpbp_ctx* c = s->ctx;
  const int E = c->E, L = c->L, qq = c->q * c->q;
  std::vector<double> h((size_t)qq * L * E);
  SCHK(s, hipMemcpy(h.data(), s->d_acc_pair, sizeof(double) * h.size(), hipMemcpyDeviceToHost));
  for (int e = 0; e < E; e++)
    for (int t = 0; t < L; t++)
      for (int k = 0; k < qq; k++) out[k + (size_t)qq * (t + (size_t)L * e)] = h[((size_t)k * L + t) * E + e] / sw;
  return MPBP_OK;
}

extern "C" int mpbp_sampler_twovar_marginals(mpbp_sampler* s, double* out) {
  if (!s || !out) return MPBP_EINVAL;
  const int nc = (int)s->sites.size();
  if (nc == 0) return s->fail(MPBP_EINVAL, "no sites for two-time marginals were requested at mpbp_sampler_create");
  double sw;
  int rc = normaliser(s, sw);
  if (rc) return rc;
  const mpbp_ctx* c = s->ctx;
  const int L = c->L, qq = c->q * c->q, D = s->D;
  const size_t n1 = (size_t)nc * L * D;
  std::vector<double> h(qq * n1);
  SCHK(s, hipMemcpy(h.data(), s->d_acc_corr, sizeof(double) * h.size(), hipMemcpyDeviceToHost));
  std::fill(out, out + (size_t)nc * L * L * qq, 0.0);
  for (int k = 0; k < nc; k++)
    for (int t = 0; t < L; t++)
      for (int u = t + 1; u < L && u <= t + D; u++)
        for (int b = 0; b < qq; b++)
          out[b + (size_t)qq * (u + (size_t)L * (t + (size_t)L * k))] = h[b * n1 + ((size_t)k * L + t) * D + (u - t - 1)] / sw;
  return MPBP_OK;
}

extern "C" int mpbp_sampler_counts(mpbp_sampler* s, int64_t* nsamples, double* log_sum_w, double* log_sum_w2) {
  if (!s) return MPBP_EINVAL;
  smp::State h{-std::numeric_limits<double>::infinity(), 0.0, 0.0, 1.0};
  if (s->count > 0) { int rc = read_state(s, h); if (rc) return rc; }
  if (nsamples) *nsamples = s->count;
  const double ninf = -std::numeric_limits<double>::infinity();
  if (log_sum_w) *log_sum_w = h.sw > 0.0 ? h.M + std::log(h.sw) : ninf;
  if (log_sum_w2) *log_sum_w2 = h.sw2 > 0.0 ? 2.0 * h.M + std::log(h.sw2) : ninf;
  return MPBP_OK;
}

extern "C" int mpbp_philox4x32_10(const uint32_t* counter, const uint32_t* key, uint32_t* out) {
  if (!counter || !key || !out) return MPBP_EINVAL;
  uint32_t c[4] = {counter[0], counter[1], counter[2], counter[3]};
  smp::philox4x32_10(c, key[0], key[1]);
  for (int k = 0; k < 4; k++) out[k] = c[k];
  return MPBP_OK;
}
