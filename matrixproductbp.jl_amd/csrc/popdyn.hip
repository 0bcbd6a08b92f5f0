// Population dynamics for the equilibrium magnetisation of the Ising model on infinite diluted graphs (reference
// src/Models/glauber/equilibrium.jl:72-127, `equilibrium_magnetization`).  C ABI: mpbp_popdyn_* in include/mpbp_hip.h.
//
// A handle owns two device arrays of popsize cavity fields, old and new.  One sweep is synchronous: member i of the new
// array is computed from the old array only,
//   km1 ~ pkm1;  h ~ ph;  for n = 0..km1-1:  a_n = min(floor(u popsize), popsize-1),  J_n ~ pJ
//   P_new[i] = (1/beta) (sum_n atanh(tanh(beta P_old[a_n]) tanh(beta J_n))) + h          (sum from 0.0 in the order n = 0, 1, ...)
// and the arrays are swapped.  The final draw is m_s = tanh(beta f) with the same f, degree ~ pk, from the current array.
//
// Random numbers: Philox4x32-10 (the block function of mpbp_philox4x32_10), key = (seed lo, seed hi),
//   counter = (member, slot, sweep, phase)
//     phase 0: the sweeps; sweep = 1, 2, ... counted over the handle's lifetime; member = index in the population
//     phase 1: the final draw; sweep = 1, 2, ... the number of the mpbp_popdyn_magnetization call; member = sample index
// One block r[0..3] gives two uniforms in [0, 1):
//   uA = ((r0 >> 5) 2^26 + (r1 >> 6)) 2^-53,   uB = ((r2 >> 5) 2^26 + (r3 >> 6)) 2^-53
//     slot 0       uA        -> degree
//     slot 1       (uA, uB)  -> field h
//     slot 2 + 2n  uA        -> index a_n
//     slot 3 + 2n  (uA, uB)  -> coupling J_n
// so a draw depends on (seed, phase, sweep, member, slot) and on nothing else - not on the launch geometry, not on how
// the caller splits mpbp_popdyn_iterate calls.  (A DIRAC distribution consumes its slot without evaluating the block.)
//
// Distributions are tables {kind, n, values[], cdf[]} computed on the host and used verbatim here:
//   DIRAC     values[0]
//   DISCRETE  values[j] of the first j with cdf[j] > uA, the last entry if there is none
//   NORMAL    values[0] + values[1] * sqrt(-2 log(1 - uA)) * cos(TWO_PI * uB)   (evaluated left to right; 1 - uA > 0)
//
// The mean of a sweep is a deterministic function of the new population alone: each 256-thread workgroup of the sweep
// kernel reduces its 256 members (0.0 beyond popsize) with the LDS tree  for s = 128, 64, .., 1: x[t] += x[t + s] (t < s)
// into one partial; one 256-thread workgroup then lets thread t add the partials t, t + 256, t + 512, ... in that order
// from 0.0, reduces the 256 sums with the same tree and divides by popsize.
//
// Deliberate differences from the reference: it updates one array in place in shuffled order and alternates between two
// arrays, here a sweep is synchronous old -> new (same fixed-point distribution, another trajectory); it draws from
// Julia's GLOBAL_RNG, here draws are counter based; it accepts any Distribution, here the three kinds above (the host
// tabulates Poisson as DISCRETE).  Arithmetic runs in fp64 with contraction off so that a host restatement reproduces it
// (tests/test_equilibrium.py).
#pragma clang fp contract(off)

#include "ctx.h"

#include <cmath>
#include <limits>
#include <new>

namespace pdy {

constexpr int NT = 256;          // threads per workgroup of every kernel here
constexpr int MAXTAB = 256;      // entries of a distribution table
constexpr double TWO_PI = 6.283185307179586;

enum { DIRAC = 0, DISCRETE = 1, NORMAL = 2 };
enum { PKM1 = 0, PK = 1, PJ = 2, PH = 3, NDIST = 4 };

struct Dist {
  int32_t kind, n;
  double values[MAXTAB];
  double cdf[MAXTAB];
};

// Random123 Philox4x32-10 (a copy of the sampler's block function: the two translation units share no host layer)
__host__ __device__ inline void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
  for (int r = 0; r < 10; r++) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0, hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
    const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
    c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
}

struct Key {
  uint64_t seed;
  uint32_t member, sweep, phase;
};

__device__ inline void uniforms(const Key& k, uint32_t slot, double& uA, double& uB) {
  uint32_t c[4] = {k.member, slot, k.sweep, k.phase};
  philox4x32_10(c, (uint32_t)k.seed, (uint32_t)(k.seed >> 32));
  uA = ((double)(c[0] >> 5) * 67108864.0 + (double)(c[1] >> 6)) * (1.0 / 9007199254740992.0);
  uB = ((double)(c[2] >> 5) * 67108864.0 + (double)(c[3] >> 6)) * (1.0 / 9007199254740992.0);
}

__device__ inline double draw(const Dist& d, const Key& k, uint32_t slot) {
  if (d.kind == DIRAC) return d.values[0];
  double uA, uB;
  uniforms(k, slot, uA, uB);
  if (d.kind == NORMAL) return d.values[0] + d.values[1] * sqrt(-2.0 * log(1.0 - uA)) * cos(TWO_PI * uB);
  const int last = d.n - 1;
  int j = 0;
  while (j < last && !(d.cdf[j] > uA)) j++;
  return d.values[j];
}

// f of equilibrium.jl:91 on `deg` members drawn from P, plus the field
__device__ inline double cavity_field(const Dist* __restrict__ tb, int which_deg, const double* __restrict__ P, int64_t n,
                                      double beta, double inv_beta, const Key& k) {
  const Dist& pJ = tb[PJ];
  const int deg = (int)draw(tb[which_deg], k, 0);
  const double h = draw(tb[PH], k, 1);
  const bool fixedJ = pJ.kind == DIRAC;
  const double tJ0 = fixedJ ? tanh(beta * pJ.values[0]) : 0.0;
  double acc = 0.0;
  for (int nn = 0; nn < deg; nn++) {
    double uA, uB;
    uniforms(k, 2u + 2u * (uint32_t)nn, uA, uB);
    int64_t a = (int64_t)floor(uA * (double)n);
    if (a > n - 1) a = n - 1;
    const double tJ = fixedJ ? tJ0 : tanh(beta * draw(pJ, k, 3u + 2u * (uint32_t)nn));
    acc += atanh(tanh(beta * P[a]) * tJ);
  }
  return inv_beta * acc + h;
}

// x[0] = sum of x[0..255] by the fixed tree; every thread of the workgroup calls it
__device__ inline void tree_sum(double* x) {
  __syncthreads();
  for (int s = NT / 2; s >= 1; s >>= 1) {
    if ((int)threadIdx.x < s) x[threadIdx.x] += x[threadIdx.x + s];
    __syncthreads();
  }
}

__global__ void __launch_bounds__(NT) k_popdyn_sweep(const Dist* __restrict__ tb, const double* __restrict__ Pold,
                                                     double* __restrict__ Pnew, int64_t n, double beta, double inv_beta,
                                                     uint64_t seed, uint32_t sweep, double* __restrict__ partial) {
  __shared__ double x[NT];
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  double v = 0.0;
  if (i < n) {
    const Key k{seed, (uint32_t)i, sweep, 0u};
    v = cavity_field(tb, PKM1, Pold, n, beta, inv_beta, k);
    Pnew[i] = v;
  }
  x[threadIdx.x] = v;
  tree_sum(x);
  if (threadIdx.x == 0) partial[blockIdx.x] = x[0];
}

__global__ void __launch_bounds__(NT) k_popdyn_mean(const double* __restrict__ partial, int64_t nblocks, int64_t n,
                                                    double* __restrict__ mean) {
  __shared__ double x[NT];
  double acc = 0.0;
  for (int64_t b = threadIdx.x; b < nblocks; b += NT) acc += partial[b];
  x[threadIdx.x] = acc;
  tree_sum(x);
  if (threadIdx.x == 0) *mean = x[0] / (double)n;
}

__global__ void __launch_bounds__(NT) k_popdyn_magnetization(const Dist* __restrict__ tb, const double* __restrict__ P,
                                                             int64_t n, double beta, double inv_beta, uint64_t seed,
                                                             uint32_t call, int64_t nsamples, double* __restrict__ m) {
  const int64_t s = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (s >= nsamples) return;
  const Key k{seed, (uint32_t)s, call, 1u};
  m[s] = tanh(beta * cavity_field(tb, PK, P, n, beta, inv_beta, k));
}

}  // namespace pdy

struct mpbp_popdyn {
  int device = 0;
  int64_t n = 0;
  uint64_t seed = 0;
  double beta = 1.0;
  uint32_t sweeps = 0, mag_calls = 0;   // sweeps done and magnetisation draws made over the handle's lifetime
  bool set[pdy::NDIST] = {false, false, false, false};
  int64_t nblocks = 0, means_cap = 0;
  pdy::Dist* d_tab = nullptr;
  double *d_cur = nullptr, *d_new = nullptr, *d_partial = nullptr, *d_means = nullptr;
};

// there is no context: the message of a failed call is read through mpbp_last_error(NULL)
static int pd_fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_create_error = buf;
  return code;
}

static int pd_hip(hipError_t e, const char* what) {
  if (e == hipSuccess) return MPBP_OK;
  return pd_fail(e == hipErrorOutOfMemory ? MPBP_ENOMEM : MPBP_EHIP, "%s failed: %s", what, hipGetErrorString(e));
}

static const char* const PD_NAMES[pdy::NDIST] = {"pkm1", "pk", "pJ", "ph"};

static int pd_need(const mpbp_popdyn* p, std::initializer_list<int> which) {
  for (int w : which)
    if (!p->set[w]) return pd_fail(MPBP_EINVAL, "distribution %s was never set (mpbp_popdyn_set_distribution)", PD_NAMES[w]);
  return MPBP_OK;
}

extern "C" void mpbp_popdyn_destroy(mpbp_popdyn* p) {
  if (!p) return;
  hipSetDevice(p->device);
  hipDeviceSynchronize();
  for (void* q : {(void*)p->d_tab, (void*)p->d_cur, (void*)p->d_new, (void*)p->d_partial, (void*)p->d_means})
    if (q) hipFree(q);
  delete p;
}

extern "C" int mpbp_popdyn_create(mpbp_popdyn** out, int32_t device, int64_t popsize, uint64_t seed, double beta,
                                  const double* P0) {
  if (!out) return pd_fail(MPBP_EINVAL, "null argument");
  *out = nullptr;
  if (popsize < 1 || popsize > 2147483647LL)
    return pd_fail(MPBP_EINVAL, "popsize must be in 1..2^31-1 (got %lld)", (long long)popsize);
  if (!(beta > 0.0) || !std::isfinite(beta)) return pd_fail(MPBP_EINVAL, "beta must be positive and finite (got %g)", beta);
  int rc;
  if ((rc = pd_hip(hipSetDevice(device), "hipSetDevice"))) return rc;
  mpbp_popdyn* p = new (std::nothrow) mpbp_popdyn();
  if (!p) return pd_fail(MPBP_ENOMEM, "host allocation failed");
  p->device = device; p->n = popsize; p->seed = seed; p->beta = beta;
  p->nblocks = (popsize + pdy::NT - 1) / pdy::NT;
  const size_t bytes = sizeof(double) * (size_t)popsize;
  if ((rc = pd_hip(hipMalloc((void**)&p->d_tab, sizeof(pdy::Dist) * pdy::NDIST), "hipMalloc(distribution tables)")) ||
      (rc = pd_hip(hipMalloc((void**)&p->d_cur, bytes), "hipMalloc(population)")) ||
      (rc = pd_hip(hipMalloc((void**)&p->d_new, bytes), "hipMalloc(population)")) ||
      (rc = pd_hip(hipMalloc((void**)&p->d_partial, sizeof(double) * (size_t)p->nblocks), "hipMalloc(partial sums)")) ||
      (rc = pd_hip(hipMemset(p->d_tab, 0, sizeof(pdy::Dist) * pdy::NDIST), "hipMemset")) ||
      (rc = pd_hip(P0 ? hipMemcpy(p->d_cur, P0, bytes, hipMemcpyHostToDevice) : hipMemset(p->d_cur, 0, bytes),
                   "population upload"))) {
    (void)hipGetLastError();
    mpbp_popdyn_destroy(p);
    return rc;
  }
  *out = p;
  return MPBP_OK;
}

extern "C" int mpbp_popdyn_set_distribution(mpbp_popdyn* p, int32_t which, int32_t kind, int32_t n, const double* values,
                                            const double* cdf) {
  if (!p) return pd_fail(MPBP_EINVAL, "null handle");
  if (which < 0 || which >= pdy::NDIST) return pd_fail(MPBP_EINVAL, "which = %d: expected 0 (pkm1), 1 (pk), 2 (pJ) or 3 (ph)", which);
  const char* nm = PD_NAMES[which];
  if (!values) return pd_fail(MPBP_EINVAL, "%s: null values", nm);
  pdy::Dist d;
  memset(&d, 0, sizeof d);
  d.kind = kind;
  const bool degree = which == pdy::PKM1 || which == pdy::PK;
  if (kind == pdy::DIRAC) {
    if (n != 1) return pd_fail(MPBP_EINVAL, "%s: a DIRAC table has 1 value (n = %d)", nm, n);
  } else if (kind == pdy::NORMAL) {
    if (degree) return pd_fail(MPBP_EINVAL, "%s: a degree distribution is DIRAC or DISCRETE", nm);
    if (n != 2) return pd_fail(MPBP_EINVAL, "%s: a NORMAL table is (mu, sigma) (n = %d)", nm, n);
    if (!(values[1] >= 0.0)) return pd_fail(MPBP_EINVAL, "%s: sigma = %g must not be negative", nm, values[1]);
  } else if (kind == pdy::DISCRETE) {
    if (n < 1 || n > pdy::MAXTAB) return pd_fail(MPBP_EINVAL, "%s: a DISCRETE table has 1..%d entries (n = %d)", nm, pdy::MAXTAB, n);
    if (!cdf) return pd_fail(MPBP_EINVAL, "%s: null cdf", nm);
    for (int j = 0; j < n; j++) {
      if (!std::isfinite(cdf[j]) || cdf[j] < 0.0 || (j > 0 && cdf[j] < cdf[j - 1]))
        return pd_fail(MPBP_EINVAL, "%s: cdf[%d] = %g: the cdf must be finite, non-negative and non-decreasing", nm, j, cdf[j]);
      d.cdf[j] = cdf[j];
    }
  } else {
    return pd_fail(MPBP_EINVAL, "%s: kind = %d: expected 0 (DIRAC), 1 (DISCRETE) or 2 (NORMAL)", nm, kind);
  }
  d.n = n;
  for (int j = 0; j < n; j++) {
    const double v = values[j];
    if (!std::isfinite(v)) return pd_fail(MPBP_EINVAL, "%s: values[%d] = %g is not finite", nm, j, v);
    if (degree && (v < 0.0 || v > 1048576.0 || v != std::floor(v)))
      return pd_fail(MPBP_EINVAL, "%s: values[%d] = %g: a degree is an integer in 0..2^20", nm, j, v);
    d.values[j] = v;
  }
  int rc;
  if ((rc = pd_hip(hipSetDevice(p->device), "hipSetDevice")) ||
      (rc = pd_hip(hipMemcpy(p->d_tab + which, &d, sizeof d, hipMemcpyHostToDevice), "distribution upload")))
    return rc;
  p->set[which] = true;
  return MPBP_OK;
}

extern "C" int mpbp_popdyn_iterate(mpbp_popdyn* p, int32_t nsweeps, double* mean_after_each) {
  if (!p) return pd_fail(MPBP_EINVAL, "null handle");
  if (nsweeps < 1) return pd_fail(MPBP_EINVAL, "nsweeps must be positive (got %d)", nsweeps);
  int rc;
  if ((rc = pd_need(p, {pdy::PKM1, pdy::PJ, pdy::PH}))) return rc;
  if ((uint64_t)p->sweeps + (uint64_t)nsweeps > 0xFFFFFFFFull)
    return pd_fail(MPBP_EINVAL, "the sweep counter of this handle is exhausted (%u sweeps done)", p->sweeps);
  if ((rc = pd_hip(hipSetDevice(p->device), "hipSetDevice"))) return rc;
  if (p->means_cap < nsweeps) {
    double* d = nullptr;
    if ((rc = pd_hip(hipMalloc((void**)&d, sizeof(double) * (size_t)nsweeps), "hipMalloc(sweep means)"))) {
      (void)hipGetLastError();
      return rc;
    }
    if (p->d_means) hipFree(p->d_means);
    p->d_means = d; p->means_cap = nsweeps;
  }
  // the sweeps are queued back to back: no host synchronisation until the means are copied out
  const double inv_beta = 1.0 / p->beta;
  for (int s = 0; s < nsweeps; s++) {
    hipLaunchKernelGGL(pdy::k_popdyn_sweep, dim3((unsigned)p->nblocks), dim3(pdy::NT), 0, 0, p->d_tab, p->d_cur, p->d_new,
                       p->n, p->beta, inv_beta, p->seed, p->sweeps + 1u + (uint32_t)s, p->d_partial);
    hipLaunchKernelGGL(pdy::k_popdyn_mean, dim3(1), dim3(pdy::NT), 0, 0, p->d_partial, p->nblocks, p->n, p->d_means + s);
    std::swap(p->d_cur, p->d_new);
  }
  p->sweeps += (uint32_t)nsweeps;
  if ((rc = pd_hip(hipGetLastError(), "population sweep launch"))) return rc;
  if (mean_after_each)
    rc = pd_hip(hipMemcpy(mean_after_each, p->d_means, sizeof(double) * (size_t)nsweeps, hipMemcpyDeviceToHost), "hipMemcpy(sweep means)");
  else
    rc = pd_hip(hipDeviceSynchronize(), "population sweep");
  return rc;
}

extern "C" int mpbp_popdyn_get_population(mpbp_popdyn* p, double* P) {
  if (!p || !P) return pd_fail(MPBP_EINVAL, "null argument");
  int rc;
  if ((rc = pd_hip(hipSetDevice(p->device), "hipSetDevice"))) return rc;
  return pd_hip(hipMemcpy(P, p->d_cur, sizeof(double) * (size_t)p->n, hipMemcpyDeviceToHost), "hipMemcpy(population)");
}

extern "C" int mpbp_popdyn_set_population(mpbp_popdyn* p, const double* P) {
  if (!p || !P) return pd_fail(MPBP_EINVAL, "null argument");
  int rc;
  if ((rc = pd_hip(hipSetDevice(p->device), "hipSetDevice"))) return rc;
  return pd_hip(hipMemcpy(p->d_cur, P, sizeof(double) * (size_t)p->n, hipMemcpyHostToDevice), "hipMemcpy(population)");
}

extern "C" int mpbp_popdyn_magnetization(mpbp_popdyn* p, int64_t nsamples, double* m) {
  if (!p) return pd_fail(MPBP_EINVAL, "null handle");
  if (nsamples < 1 || nsamples > 2147483647LL)
    return pd_fail(MPBP_EINVAL, "nsamples must be in 1..2^31-1 (got %lld)", (long long)nsamples);
  if (!m) return pd_fail(MPBP_EINVAL, "null output");
  int rc;
  if ((rc = pd_need(p, {pdy::PK, pdy::PJ, pdy::PH}))) return rc;
  if (p->mag_calls == 0xFFFFFFFFu) return pd_fail(MPBP_EINVAL, "the draw counter of this handle is exhausted");
  if ((rc = pd_hip(hipSetDevice(p->device), "hipSetDevice"))) return rc;
  double* d_m = nullptr;
  if ((rc = pd_hip(hipMalloc((void**)&d_m, sizeof(double) * (size_t)nsamples), "hipMalloc(magnetisation samples)"))) {
    (void)hipGetLastError();
    return rc;
  }
  const unsigned nb = (unsigned)((nsamples + pdy::NT - 1) / pdy::NT);
  hipLaunchKernelGGL(pdy::k_popdyn_magnetization, dim3(nb), dim3(pdy::NT), 0, 0, p->d_tab, p->d_cur, p->n, p->beta,
                     1.0 / p->beta, p->seed, p->mag_calls + 1u, nsamples, d_m);
  p->mag_calls += 1u;
  if (!(rc = pd_hip(hipGetLastError(), "magnetisation launch")))
    rc = pd_hip(hipMemcpy(m, d_m, sizeof(double) * (size_t)nsamples, hipMemcpyDeviceToHost), "hipMemcpy(magnetisation samples)");
  hipFree(d_m);
  return rc;
}
