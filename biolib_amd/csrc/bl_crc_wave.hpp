// bl_crc_wave.hpp — CRC-32 (the gzip polynomial) of one BGZF member's text by one wave, shared by the inflate and the deflate units.
// The lanes take 64 consecutive slices, each its slice's own CRC; the CRC of a concatenation is
//   crc(A || B) = crc(A) * x^(8 |B|) + crc(B)  (mod P),
// so lane i's value is carried over the bytes behind its slice and the 64 results are added (xor) by the caller.
// Compiles for gfx950 and, under BL_CPU_EMU, for the host (tests/emu/emu_deflate.cpp).  Internal.
#pragma once
#include <cstdint>

#if defined(BL_CPU_EMU)
#define BL_CRC_DEV inline
#define BL_CRC_HD constexpr
#define BL_CRC_CONST static const
#else
#define BL_CRC_DEV __device__ __forceinline__
#define BL_CRC_HD __host__ __device__ constexpr
#define BL_CRC_CONST static __constant__
#endif

namespace blcrcw {

constexpr uint32_t CRC_POLY = 0xedb88320u;  // CRC-32 of gzip, bit-reflected: bit 31 of a word is x^0

// a(x) * b(x) mod P(x) in the reflected representation
BL_CRC_HD uint32_t mulmod(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (int i = 0; i < 32; ++i) {
        if (a & (0x80000000u >> i)) p ^= b;
        b = (b >> 1) ^ ((b & 1u) ? CRC_POLY : 0u);
    }
    return p;
}

struct PowerTable {
    uint32_t x2n[32];  // x^(2^k) mod P
};
constexpr PowerTable make_powers()
{
    PowerTable t{};
    uint32_t p = 0x40000000u;  // x^1
    for (int k = 0; k < 32; ++k) {
        t.x2n[k] = p;
        p = mulmod(p, p);
    }
    return t;
}
BL_CRC_CONST PowerTable g_powers = make_powers();

// entries lane, lane + 64, ... of the byte table (256 words); the caller synchronises before the table is read
BL_CRC_DEV void fill_table(uint32_t* table, uint32_t lane)
{
    for (uint32_t e = lane; e < 256; e += 64) {
        uint32_t c = e;
        for (int k = 0; k < 8; ++k) c = (c >> 1) ^ ((c & 1u) ? CRC_POLY : 0u);
        table[e] = c;
    }
}

// lane's share of the CRC-32 of p[0, isize): the xor over the 64 lanes is the CRC
BL_CRC_DEV uint32_t lane_share(const uint32_t* table, const uint8_t* p, uint32_t isize, uint32_t lane)
{
    const uint32_t slice = (isize + 63u) / 64u;
    const uint32_t a = lane * slice < isize ? lane * slice : isize;
    const uint32_t b = a + slice < isize ? a + slice : isize;
    uint32_t c = 0xffffffffu;
    uint32_t i = a;
    for (; i + 8 <= b; i += 8) {  // 8 bytes a load, whatever the alignment
        uint64_t w;
        __builtin_memcpy(&w, p + i, 8);
        for (int k = 0; k < 8; ++k) c = table[(c ^ (uint32_t)(w >> (8 * k))) & 0xffu] ^ (c >> 8);
    }
    for (; i < b; ++i) c = table[(c ^ p[i]) & 0xffu] ^ (c >> 8);
    c = a < b ? ~c : 0u;
    uint32_t power = 0x80000000u;  // x^0, then x^(8 * bytes behind the slice)
    uint32_t behind = isize - b;
    for (int k = 3; behind; ++k, behind >>= 1)
        if (behind & 1u) power = mulmod(g_powers.x2n[k & 31], power);
    return mulmod(power, c);
}

}  // namespace blcrcw
