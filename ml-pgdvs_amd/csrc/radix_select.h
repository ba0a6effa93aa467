// Exact order statistics of a device array of float / double keys, as numpy's partition orders them: an MSB-first radix
// select over the keys' order-preserving bit patterns (11-bit digits: 3 passes for float, 6 for double; -0.0 counted as
// +0.0), shared by the loaders' depth-range ops (depth_range.hip).
//
// NR ranks run together: a histogram pass counts each key into the slot of the rank whose prefix it matches (ranks with
// equal prefixes share a slot, distinct prefixes are disjoint, so one LDS atomic per key at most), a one-block pass of
// NR wavefronts picks every rank's digit.  After the last pass, Key<T>::dec(prefix[r]) is the value of rank r.
#pragma once
#include <cmath>

#include "common.h"
#include "wave.h"

namespace pgdvs {
namespace radix {
namespace {

constexpr int kDigit = 11, kBins = 1 << kDigit, kBlock = 256;

template <typename T> struct Key;
template <> struct Key<float> {
  typedef uint32_t U;
  static constexpr int kBits = 32;
  __device__ static U enc(float f) {
    uint32_t u = __float_as_uint(f == 0.0f ? 0.0f : f);  // -0.0 and +0.0 compare equal in numpy's partition
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  }
  __device__ static float dec(U k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
};
template <> struct Key<double> {
  typedef uint64_t U;
  static constexpr int kBits = 64;
  __device__ static U enc(double f) {
    uint64_t u = (uint64_t)__double_as_longlong(f == 0.0 ? 0.0 : f);
    return (u >> 63) ? ~u : (u | (1ull << 63));
  }
  __device__ static double dec(U k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & ~(1ull << 63)) : ~k));
  }
};

inline int passes_for(int key_bits) { return (key_bits + kDigit - 1) / kDigit; }

// the select's device state; set by init, advanced by every select pass
template <int NR> struct Sel {
  unsigned long long prefix[NR];
  uint32_t rem[NR];
  int32_t slot[NR];
};

// every rank starts in slot 0 with an empty prefix (one shared first pass); remaining rank = the rank itself
template <int NR> __device__ void sel_init(Sel<NR> *st, const int64_t *rank) {
  for (int r = 0; r < NR; ++r) {
    st->prefix[r] = 0;
    st->rem[r] = (uint32_t)rank[r];
    st->slot[r] = 0;
  }
}

template <typename T, int NR>
__global__ void __launch_bounds__(kBlock) hist_kernel(const typename Key<T>::U *__restrict__ keys, int64_t n, int pass,
                                                      const Sel<NR> *__restrict__ st, uint32_t *__restrict__ hist) {
  typedef typename Key<T>::U U;
  __shared__ uint32_t h[NR][kBins];
  for (int k = threadIdx.x; k < NR * kBins; k += kBlock) (&h[0][0])[k] = 0;
  const int kb = Key<T>::kBits;
  const int shift = kb - kDigit * (pass + 1) > 0 ? kb - kDigit * (pass + 1) : 0;
  const int hs = kb - kDigit * pass;  // bits above this pass's digit: the prefix
  bool act[NR];
  U pre[NR];
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    act[r] = st->slot[r] == r;
    pre[r] = (U)st->prefix[r];
  }
  __syncthreads();
  const U dmask = (U)((1u << (hs - shift)) - 1u);
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    const U k = keys[i];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      if (act[r] && (pass == 0 || (k >> hs) == pre[r])) {
        atomicAdd(&h[r][(int)((k >> shift) & dmask)], 1u);
        break;
      }
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < NR * kBins; k += kBlock) {
    const uint32_t c = (&h[0][0])[k];
    if (c) atomicAdd(&hist[k], c);
  }
}

// grid-stride launch size of hist_kernel over n keys
inline unsigned hist_grid(int64_t n) { return (unsigned)std::min<int64_t>(cdiv(n, kBlock * 16), 1024); }

// Called by every thread of a one-block kernel of NR * 64 threads: picks this pass's digit of every rank from the
// pass's histograms and regroups the ranks into slots.  On return (after a block barrier) st holds the new prefixes.
template <typename T, int NR> __device__ void select_digits(int pass, Sel<NR> *st, const uint32_t *__restrict__ hist) {
  typedef typename Key<T>::U U;
  const int r = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int kb = Key<T>::kBits;
  const int shift = kb - kDigit * (pass + 1) > 0 ? kb - kDigit * (pass + 1) : 0;
  const int width = kb - kDigit * pass - shift;
  const uint32_t *h = hist + (size_t)st->slot[r] * kBins;
  const uint32_t rem = st->rem[r];
  constexpr int kPer = kBins / 64;
  uint32_t c = 0;
  for (int b = 0; b < kPer; ++b) c += h[lane * kPer + b];
  const uint32_t incl = wave_incl_scan(c);
  const uint32_t excl = incl - c;
  const unsigned long long hit = __ballot(excl <= rem && rem < incl);
  const int L = hit ? __builtin_ctzll(hit) : 63;  // always hit: rem < n = total count of the slot
  int digit = 0;
  uint32_t nrem = 0;
  if (lane == L) {
    uint32_t cum = excl;
    for (int b = 0; b < kPer; ++b) {
      const uint32_t hb = h[lane * kPer + b];
      if (rem < cum + hb) {
        digit = lane * kPer + b;
        nrem = rem - cum;
        break;
      }
      cum += hb;
    }
  }
  digit = __shfl(digit, L, 64);
  nrem = __shfl(nrem, L, 64);
  __syncthreads();  // every wave has read the old state
  if (lane == 0) {
    const U old = pass == 0 ? (U)0 : (U)st->prefix[r];
    st->prefix[r] = (unsigned long long)((old << width) | (U)digit);
    st->rem[r] = nrem;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int a = 0; a < NR; ++a) {
      int s = a;
      for (int b = 0; b < a; ++b)
        if (st->prefix[b] == st->prefix[a]) {
          s = b;
          break;
        }
      st->slot[a] = s;
    }
  }
  __syncthreads();
}

template <typename T, int NR> __device__ T rank_value(const Sel<NR> *st, int r) {
  return Key<T>::dec((typename Key<T>::U)st->prefix[r]);
}

// numpy's _lerp: a + (b - a) t, or b - (b - a)(1 - t) where t >= 0.5 (all in T, no contraction)
template <typename T> __device__ T lerp_np(T a, T b, T t) {
  const T diff = b - a;
  T r = a + diff * t;
  if (t >= (T)0.5) r = b - diff * ((T)1 - t);
  return r;
}

// numpy's linear-method virtual index in T: (n - 1) q, the neighbours floor / floor + 1 (both the last element when the
// index reaches n - 1), gamma = index - floor (numpy forms it in float64, then casts to T)
template <typename T> void quantile_setup(int64_t n, T q, int64_t &a, int64_t &b, T &gamma) {
  const T vi = (T)(n - 1) * q;
  if (vi >= (T)(n - 1)) {
    a = b = n - 1;
    gamma = (T)((double)vi + 1.0);
    return;
  }
  const T prev = std::floor(vi);
  a = (int64_t)prev;
  b = (int64_t)(prev + (T)1);
  gamma = (T)((double)vi - (double)a);
}

}  // namespace
}  // namespace radix
}  // namespace pgdvs
