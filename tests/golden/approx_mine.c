/* Helper of make_approx_adversaries.py, compiled when the generator runs: the searches numpy is too slow for.  Written from the same rule
 * as tests/hash_top_model.py (the generator checks every hit against that model):
 *   hash64 = F1 + F2, the two finalised lanes of MurmurHash3_x64_128 over one 8-byte key;  S = hi(F1) + hi(F2),  carry = (lo(F1) + lo(F2)) >> 32.
 * A wrap is S == 0xffffffff: 2^-32 per key. */
#include <stdint.h>

static inline uint64_t fmix(uint64_t x)
{
    x ^= x >> 33;
    x *= 0xff51afd7ed558ccdULL;
    x ^= x >> 33;
    x *= 0xc4ceb9fe1a85ec53ULL;
    return x ^ (x >> 33);
}

static inline void top_carry(uint64_t key, uint32_t seed, uint32_t* s, uint32_t* carry)
{
    uint64_t k = key * 0x87c37b91114253d5ULL;
    k = (k << 31) | (k >> 33);
    k *= 0x4cf5ad432745937fULL;
    uint64_t h1 = ((uint64_t)seed ^ k) ^ 8, h2 = (uint64_t)seed ^ 8;
    h1 += h2;
    h2 += h1;
    const uint64_t f1 = fmix(h1), f2 = fmix(h2);
    *s = (uint32_t)(f1 >> 32) + (uint32_t)(f2 >> 32);
    *carry = (uint32_t)(((f1 & 0xffffffffULL) + (f2 & 0xffffffffULL)) >> 32);
}

static inline uint64_t splitmix(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ULL;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
    return x ^ (x >> 31);
}

/* reverse complement of a 2-bit packed string of `len` bases (first base most significant) */
static inline uint64_t revcomp(uint64_t v, int len)
{
    uint64_t x = ~v;
    x = ((x >> 2) & 0x3333333333333333ULL) | ((x & 0x3333333333333333ULL) << 2);
    x = ((x >> 4) & 0x0f0f0f0f0f0f0f0fULL) | ((x & 0x0f0f0f0f0f0f0f0fULL) << 4);
    x = __builtin_bswap64(x);
    return x >> (64 - 2 * len);
}

/* Canonical 31-mers drawn as splitmix(counter) >> 2, counters [start, start + count): the first one whose S is 0xffffffff with carry c goes
 * to out[c] (key) and at[c] (counter); entries stay ~0 where the range holds none. */
void mine_wrap31(uint32_t seed, uint64_t start, uint64_t count, uint64_t* out, uint64_t* at)
{
    out[0] = out[1] = at[0] = at[1] = ~0ULL;
    for (uint64_t c = start; c < start + count; ++c) {
        const uint64_t v = splitmix(c) >> 2, r = revcomp(v, 31), k = v < r ? v : r;
        uint32_t s, cy;
        top_carry(k, seed, &s, &cy);
        if (s == 0xffffffffu && at[cy] == ~0ULL) {
            out[cy] = k;
            at[cy] = c;
        }
    }
}

/* Every string of `len` bases (len <= 16) under the seeds [seed0, seed0 + n): the first (seed, key) whose S is 0xffffffff with carry c goes to
 * seed_out[c], key_out[c]; ~0 where there is none. */
void mine_wrap_small(int len, uint32_t seed0, uint32_t n, uint64_t* seed_out, uint64_t* key_out)
{
    seed_out[0] = seed_out[1] = key_out[0] = key_out[1] = ~0ULL;
    const uint64_t space = 1ULL << (2 * len);
    for (uint32_t i = 0; i < n; ++i) {
        for (uint64_t k = 0; k < space; ++k) {
            uint32_t s, cy;
            top_carry(k, seed0 + i, &s, &cy);
            if (s == 0xffffffffu && seed_out[cy] == ~0ULL) {
                seed_out[cy] = seed0 + i;
                key_out[cy] = k;
            }
        }
    }
}
