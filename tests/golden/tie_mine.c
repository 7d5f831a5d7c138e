/* Helper of make_tie_adversaries.py, compiled when the generator runs.  Written from the rule of tests/hash_top_model.py (the generator checks every
 * hit against that model): hash64 = the two finalised lanes of MurmurHash3_x64_128 over one 8-byte key, added.
 *
 * One search: a string of unit + w - 1 bases whose units at the offsets pi < pj hash smallest of its w units, tie in what a fast form keeps and
 * differ in what it drops.  d = pj - pi.  Overlapping units (d < unit): fix the unit - d bases they share, take a table of left and a table of
 * right extensions; units apart (d >= unit): fix the d - unit bases between them and take two tables of whole units.  A table holds every
 * extension when there are at most 2^log_table of them, else 2^log_table drawn ones.  Only hashes in the lowest 2 / w of the range are kept
 * (they have to be the minima of w units), the right table is sorted, the left one joined against it on the kept bits, and the bases before and
 * after the pair are drawn until every other unit hashes above the pair in its top 25 bits already. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

static inline uint64_t fmix(uint64_t x)
{
    x ^= x >> 33;
    x *= 0xff51afd7ed558ccdULL;
    x ^= x >> 33;
    x *= 0xc4ceb9fe1a85ec53ULL;
    return x ^ (x >> 33);
}

static inline uint64_t hash64(uint64_t key, uint32_t seed)
{
    uint64_t k = key * 0x87c37b91114253d5ULL;
    k = (k << 31) | (k >> 33);
    k *= 0x4cf5ad432745937fULL;
    uint64_t h1 = ((uint64_t)seed ^ k) ^ 8, h2 = (uint64_t)seed ^ 8;
    h1 += h2;
    h2 += h1;
    return fmix(h1) + fmix(h2);
}

static inline uint64_t splitmix(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ULL;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
    return x ^ (x >> 31);
}

static inline uint64_t rnd(uint64_t* s) { return splitmix((*s)++); }

/* reverse complement of a 2-bit packed string of `len` bases (first base most significant) */
static inline uint64_t revcomp(uint64_t v, int len)
{
    uint64_t x = ~v;
    x = ((x >> 2) & 0x3333333333333333ULL) | ((x & 0x3333333333333333ULL) << 2);
    x = ((x >> 4) & 0x0f0f0f0f0f0f0f0fULL) | ((x & 0x0f0f0f0f0f0f0f0fULL) << 4);
    x = __builtin_bswap64(x);
    return x >> (64 - 2 * len);
}

static inline uint64_t mask2(int bases) { return bases >= 32 ? ~0ULL : ((1ULL << (2 * bases)) - 1); }

static inline uint64_t unit_key(uint64_t v, int unit, int canon)
{
    if (!canon) return v;
    const uint64_t r = revcomp(v, unit);
    return v < r ? v : r;
}

typedef struct {
    uint64_t h;
    uint64_t v;
} ent;

static int cmp_ent(const void* a, const void* b)
{
    const ent *x = (const ent*)a, *y = (const ent*)b;
    if (x->h != y->h) return x->h < y->h ? -1 : 1;
    return x->v < y->v ? -1 : (x->v > y->v);
}

/* cls 0: p26 (bits 63..38 equal, the high dwords differ)   1: p25 (bits 63..39 equal, bit 38 differs)   2: hi32 (high dwords equal, low ones differ) */
static const int SHIFT[3] = {38, 39, 32};
static int tied(uint64_t a, uint64_t b, int cls)
{
    if (a == b) return 0;
    if (cls == 0) return (a >> 38) == (b >> 38) && (a >> 32) != (b >> 32);
    if (cls == 1) return (a >> 39) == (b >> 39) && (((a ^ b) >> 38) & 1);
    return (a >> 32) == (b >> 32);
}

static void put(uint8_t* dst, uint64_t v, int bases)
{
    for (int i = 0; i < bases; ++i) dst[i] = (uint8_t)((v >> (2 * (bases - 1 - i))) & 3);
}

static uint64_t value_at(const uint8_t* c, int bases)
{
    uint64_t v = 0;
    for (int i = 0; i < bases; ++i) v = (v << 2) | c[i];
    return v;
}

/* Counters [c0, c0 + count), each its own generator state: the first hit whose smaller hash is the unit at pi goes to out[0 ..] (2-bit codes,
 * unit + w - 1 of them) and at[0] (its counter), the first whose smaller hash is at pj to out[span ..] and at[1]; at[] stays ~0 without one.
 * kcanon: the whole string, read as one (unit + w - 1 <= 32)-mer, must be smaller than its reverse complement.
 * guard (pi = 0): a hit whose smaller hash is at pj also needs a base g such that the unit that starts one base earlier, g and the string's first
 * unit - 1 bases, hashes below the unit at 0 in its top 25 bits: with g planted in front, no window of a longer sequence elects the unit at 0, and
 * a scan that takes it for the string's own window reports a record too many.  g goes to out[2 * span + side] (255: none asked for). */
void tie_mine(int unit, int w, uint32_t seed, int canon, int cls, int pi, int pj, int kcanon, int guard, int log_table, uint64_t c0, uint64_t count,
              uint8_t* out, uint64_t* at)
{
    const int span = unit + w - 1, d = pj - pi, e = d < unit ? d : unit, fixed = d < unit ? unit - d : d - unit;
    const int all = 2 * e <= log_table;
    const size_t nt = (size_t)1 << (all ? 2 * e : log_table);
    const uint64_t tau = w <= 2 ? ~0ULL : (~0ULL / (uint64_t)w) * 2;
    const int tries = (pi == 0 && pj == w - 1) ? 1 : 32;
    ent* la = (ent*)malloc(nt * sizeof(ent));
    ent* lb = (ent*)malloc(nt * sizeof(ent));
    at[0] = at[1] = ~0ULL;
    for (uint64_t c = c0; c < c0 + count && (at[0] == ~0ULL || at[1] == ~0ULL); ++c) {
        uint64_t s = splitmix(c) << 8;
        const uint64_t fix = rnd(&s) & mask2(fixed);
        size_t na = 0, nb = 0;
        for (size_t x = 0; x < nt; ++x) {
            const uint64_t xe = all ? (uint64_t)x : (rnd(&s) & mask2(e)), ye = all ? (uint64_t)x : (rnd(&s) & mask2(e));
            const uint64_t a = d < unit ? ((xe << (2 * fixed)) | fix) : xe, b = d < unit ? ((fix << (2 * d)) | ye) : ye;
            const uint64_t ha = hash64(unit_key(a, unit, canon), seed), hb = hash64(unit_key(b, unit, canon), seed);
            if (ha <= tau) la[na++] = (ent){ha, xe};
            if (hb <= tau) lb[nb++] = (ent){hb, ye};
        }
        if (!na || !nb) continue;
        if (nb <= 16) {
            for (size_t i = 1; i < nb; ++i) {
                const ent t = lb[i];
                size_t j = i;
                for (; j > 0 && cmp_ent(&lb[j - 1], &t) > 0; --j) lb[j] = lb[j - 1];
                lb[j] = t;
            }
        } else {
            qsort(lb, nb, sizeof(ent), cmp_ent);
        }
        for (size_t i = 0; i < na; ++i) {
            const uint64_t key = la[i].h >> SHIFT[cls];
            size_t lo = 0, hi = nb;
            while (lo < hi) {
                const size_t m = (lo + hi) / 2;
                if ((lb[m].h >> SHIFT[cls]) < key) lo = m + 1;
                else hi = m;
            }
            for (size_t t = lo; t < nb && (lb[t].h >> SHIFT[cls]) == key; ++t) {
                if (!tied(la[i].h, lb[t].h, cls)) continue;
                const int side = la[i].h < lb[t].h ? 0 : 1;
                if (at[side] != ~0ULL) continue;
                uint8_t win[160];
                const uint64_t top = (la[i].h > lb[t].h ? la[i].h : lb[t].h) >> 39;
                for (int f = 0; f < tries; ++f) {
                    for (int x = 0; x < pi; ++x) win[x] = (uint8_t)(rnd(&s) & 3);
                    uint8_t* blk = win + pi;
                    if (d < unit) {
                        put(blk, la[i].v, d);
                        put(blk + d, fix, fixed);
                        put(blk + unit, lb[t].v, d);
                    } else {
                        put(blk, la[i].v, unit);
                        put(blk + unit, fix, fixed);
                        put(blk + d, lb[t].v, unit);
                    }
                    for (int x = pj + unit; x < span; ++x) win[x] = (uint8_t)(rnd(&s) & 3);
                    int ok = 1;
                    for (int x = 0; x < w && ok; ++x) {
                        const uint64_t h = hash64(unit_key(value_at(win + x, unit), unit, canon), seed);
                        if (x == pi) ok = h == la[i].h;
                        else if (x == pj) ok = h == lb[t].h;
                        else ok = (h >> 39) > top;
                    }
                    if (ok && kcanon) {
                        const uint64_t k = value_at(win, span);
                        ok = k < revcomp(k, span);
                    }
                    uint8_t g = 255;
                    if (ok && guard && side == 1) {
                        const uint64_t head = value_at(win, unit - 1);
                        for (uint64_t x = 0; x < 4 && g == 255; ++x)
                            if ((hash64(unit_key((x << (2 * (unit - 1))) | head, unit, canon), seed) >> 39) < (la[i].h >> 39)) g = (uint8_t)x;
                        ok = g != 255;
                    }
                    if (ok) {
                        out[2 * span + side] = g;
                        memcpy(out + (size_t)side * span, win, (size_t)span);
                        at[side] = c;
                        break;
                    }
                }
            }
        }
    }
    free(la);
    free(lb);
}
