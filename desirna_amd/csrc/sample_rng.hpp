// sample_rng.hpp -- the random numbers of the stochastic traceback (fold_sample.hpp): a counter-based function without state,
// shared by the kernel, its CPU emulation and the host.  Plain C++, no library.  Part of the contract:
//
//   mix(z)          = z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31   (SplitMix64's finalizer)
//   bits(seed,s,k)  = mix(mix(mix(seed + G) + (s + 1) G) + (k + 1) G),   G = 0x9E3779B97F4A7C15, all arithmetic mod 2^64
//   u(seed,s,k)     = (bits >> 11) * 2^-53                                a double in [0, 1) with 53 bits
//
// seed: the sequence's seed, s: the sample's index, k: the draw's index within the sample.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DRNA_RNG_HD __host__ __device__
#else
#define DRNA_RNG_HD
#endif

namespace drna {

DRNA_RNG_HD inline uint64_t sample_mix64(uint64_t z) {
  z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27; z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}

// the state of sample s of a sequence: sample_u() of it and the draw's index gives the draw
DRNA_RNG_HD inline uint64_t sample_key(uint64_t seed, uint64_t s) {
  const uint64_t G = 0x9E3779B97F4A7C15ull;
  return sample_mix64(sample_mix64(seed + G) + (s + 1) * G);
}
DRNA_RNG_HD inline double sample_u_key(uint64_t key, uint64_t k) {
  const uint64_t G = 0x9E3779B97F4A7C15ull;
  return (double)(sample_mix64(key + (k + 1) * G) >> 11) * (1.0 / 9007199254740992.0);
}
DRNA_RNG_HD inline double sample_u(uint64_t seed, uint64_t s, uint64_t k) { return sample_u_key(sample_key(seed, s), k); }

}  // namespace drna
