// The keyed bijection of [0, n) shared by the hard-ray pool's row choice (r2l_pool.hip) and the ray store's shuffle and sampler
// (r2l_raystore.hip): a 4-round Feistel network on the next even number of bits, cycle-walked back into the range.
//   bits      = the smallest even number >= 2 with 2^bits >= n            (the domain is < 4 n: ~2 trips on average at worst)
//   round keys k[0..3] from the 64-bit key                                 (perm_round_keys)
//   pi(key, n)(i) = the first of F(i), F(F(i)), ... that is < n, F = the Feistel network on bits / 2 + bits / 2 bits
// r2l_amd/raystore.py restates it in numpy (perm); tests hold the two together bit for bit.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define R2L_PERM_HD __host__ __device__ __forceinline__
#else
#define R2L_PERM_HD inline
#endif

R2L_PERM_HD unsigned perm_mix(unsigned x) {  // murmur3 finalizer
    x ^= x >> 16; x *= 0x85ebca6bu; x ^= x >> 13; x *= 0xc2b2ae35u; x ^= x >> 16;
    return x;
}

R2L_PERM_HD void perm_round_keys(unsigned long long key, unsigned (&k)[4]) {
    k[0] = perm_mix((unsigned)key);
    k[1] = perm_mix((unsigned)(key >> 32) ^ 0x9e3779b9u);
    k[2] = perm_mix((unsigned)key ^ 0x7f4a7c15u);
    k[3] = perm_mix((unsigned)(key >> 32) + 0x6a09e667u);
}

// bijection of [0, 2^(2*half_bits)): 4 Feistel rounds with round keys k[r]
R2L_PERM_HD unsigned long long perm_feistel(unsigned long long x, int half_bits, const unsigned (&k)[4]) {
    const unsigned mask = (1u << half_bits) - 1u;
    unsigned l = (unsigned)(x >> half_bits) & mask, r = (unsigned)x & mask;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const unsigned f = perm_mix(r ^ k[i]) & mask;
        const unsigned nl = r;
        r = l ^ f;
        l = nl;
    }
    return ((unsigned long long)l << half_bits) | r;
}

// pi(i) for i < n; half_bits = perm_half_bits(n)
R2L_PERM_HD unsigned long long perm_at(unsigned long long i, unsigned long long n, int half_bits, const unsigned (&k)[4]) {
    unsigned long long x = i;
    do {
        x = perm_feistel(x, half_bits, k);  // cycle walking
    } while (x >= n);
    return x;
}

R2L_PERM_HD int perm_half_bits(long long n) {
    int bits = 2;
    while (((long long)1 << bits) < n) bits += 2;  // even, 2^bits >= n, < 4 n
    return bits / 2;
}

// Key of epoch e of the ray store's sampler: the splitmix64 finalizer of seed + (e + 1) * 0x9E3779B97F4A7C15 (mod 2^64).
R2L_PERM_HD unsigned long long perm_epoch_key(unsigned long long seed, unsigned long long epoch) {
    unsigned long long z = seed + (epoch + 1ull) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
