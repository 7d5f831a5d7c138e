// TEST INFRASTRUCTURE: the wave-per-member DEFLATE encoder of biolib_amd/csrc/bl_deflate_core.hpp compiled for the host (lane loops
// instead of lanes, arrays instead of LDS) and run the way bl_bgzf_deflate runs it: members into slots, an exclusive sum of their
// sizes, the gather into the output, the EOF marker.  Built with -fsanitize=address,undefined by tests/test_emu_deflate.py.
//
//   emu_deflate TEXT_FILE N_BYTES EOF(0|1) OUT_PREFIX
// The text is placed `align` bytes into an allocation of exactly align + N_BYTES bytes (16-byte aligned: the text's first byte at every
// alignment 0..15 in turn, its last byte the allocation's last, which the sanitizer guards to the byte); the output
// has exactly bl_bgzf_bound bytes.  All 16 runs must give the same bytes; they are inflated again with zlib and compared with the
// text.  Writes OUT_PREFIX.bgzf and OUT_PREFIX.members (bl_bgzf_member rows) and prints
//   n_out n_members stored fixed dynamic limited max_len min_len max_dist min_dist
#include <zlib.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/biolib_amd.h"
#include "../../biolib_amd/csrc/bl_deflate_core.hpp"

namespace {

const unsigned char EOF_MARKER[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};

uint64_t bound(uint64_t n, bool eof) { return n + 31 * ((n + bl_deflate::MEMBER_TEXT - 1) / bl_deflate::MEMBER_TEXT) + (eof ? 28 : 0); }

struct Run {
    std::vector<uint8_t> out;
    std::vector<bl_bgzf_member> members;
    bl_deflate::Stats stats;
    bool ok = true;
};

Run run(const std::vector<uint8_t>& text, bool eof, unsigned align)
{
    using namespace bl_deflate;
    Run r;
    const uint64_t n = text.size(), n_members = (n + MEMBER_TEXT - 1) / MEMBER_TEXT, cap = bound(n, eof);
    // a block of exactly align + n bytes: malloc's blocks begin 16-byte aligned, so the text's first byte sits at alignment `align`, and
    // AddressSanitizer poisons what lies behind a block's last byte to the byte, so the text ends where the readable memory ends
    uint8_t* exact = static_cast<uint8_t*>(std::malloc(align + n ? align + n : 1));
    if (reinterpret_cast<uintptr_t>(exact) & 15u) {
        std::free(exact);
        r.ok = false;  // (the premise of the run)
        return r;
    }
    uint8_t* t = exact + align;
    if (n) std::memcpy(t, text.data(), n);
    uint8_t* out = static_cast<uint8_t*>(std::malloc(cap ? cap : 1));
    std::memset(out, 0xA5, cap ? cap : 1);
    static Shared sh;
    std::vector<uint32_t> tokens(MAX_TOKENS + 1);
    std::vector<uint8_t*> slots(n_members);
    std::vector<uint32_t> sizes(n_members), crcs(n_members);
    for (uint64_t m = 0; m < n_members; ++m) {
        slots[m] = static_cast<uint8_t*>(std::aligned_alloc(64, SLOT_BYTES));
        const uint32_t len = (uint32_t)(n - m * MEMBER_TEXT < MEMBER_TEXT ? n - m * MEMBER_TEXT : MEMBER_TEXT);
        sizes[m] = deflate_member(sh, t + m * MEMBER_TEXT, len, tokens.data(), slots[m], crcs[m], &r.stats);
        if (sizes[m] == 0 || sizes[m] > len + MEMBER_OVERHEAD) r.ok = false;
    }
    uint64_t at = 0;
    for (uint64_t m = 0; m < n_members && r.ok; ++m) {
        for (uint32_t th = 0; th < 256; ++th) gather_member(slots[m], out + at, sizes[m], th, 256);
        bl_bgzf_member row;
        row.src_off = at + 18;
        row.dst_off = m * MEMBER_TEXT;
        row.src_len = sizes[m] - 26;
        row.isize = (uint32_t)(n - m * MEMBER_TEXT < MEMBER_TEXT ? n - m * MEMBER_TEXT : MEMBER_TEXT);
        row.crc = crcs[m];
        row.reserved = 0;
        r.members.push_back(row);
        at += sizes[m];
    }
    if (eof && r.ok) {
        std::memcpy(out + at, EOF_MARKER, 28);
        at += 28;
    }
    if (at > cap) r.ok = false;
    for (uint64_t i = at; i < cap; ++i)
        if (out[i] != 0xA5) r.ok = false;  // nothing at or behind the end
    r.out.assign(out, out + at);
    for (auto* s : slots) std::free(s);
    std::free(out);
    std::free(exact);
    return r;
}

// every member inflated with zlib: the text again?
bool inflates_to(const Run& r, const std::vector<uint8_t>& text)
{
    std::vector<uint8_t> back(text.size() + 1);
    for (const auto& m : r.members) {
        z_stream z;
        std::memset(&z, 0, sizeof(z));
        if (inflateInit2(&z, -15) != Z_OK) return false;
        z.next_in = const_cast<uint8_t*>(r.out.data() + m.src_off);
        z.avail_in = m.src_len;
        z.next_out = back.data() + m.dst_off;
        z.avail_out = m.isize;
        const int rc = inflate(&z, Z_FINISH);
        const bool good = rc == Z_STREAM_END && z.total_out == m.isize && z.avail_in == 0;
        inflateEnd(&z);
        if (!good) return false;
        if ((uint32_t)crc32(0, back.data() + m.dst_off, m.isize) != m.crc) return false;
    }
    return text.empty() || std::memcmp(back.data(), text.data(), text.size()) == 0;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 5) return 2;
    const uint64_t n = std::strtoull(argv[2], nullptr, 10);
    const bool eof = std::atoi(argv[3]) != 0;
    std::vector<uint8_t> text(n);
    if (n) {
        FILE* f = std::fopen(argv[1], "rb");
        if (!f || std::fread(text.data(), 1, n, f) != n) return 2;
        std::fclose(f);
    }
    Run first;
    for (unsigned align = 0; align < 16; ++align) {
        Run r = run(text, eof, align);
        if (!r.ok) {
            std::printf("FAIL: a member's size, or a byte behind the output, at alignment %u\n", align);
            return 1;
        }
        if (align == 0) {
            first = r;
            if (!inflates_to(first, text)) {
                std::printf("FAIL: zlib does not give the text back\n");
                return 1;
            }
        } else if (r.out != first.out || r.members.size() != first.members.size() ||
                   (!r.members.empty() && std::memcmp(r.members.data(), first.members.data(), r.members.size() * sizeof(bl_bgzf_member)) != 0)) {
            std::printf("FAIL: alignment %u gives other bytes than alignment 0\n", align);
            return 1;
        }
    }
    const std::string prefix = argv[4];
    FILE* f = std::fopen((prefix + ".bgzf").c_str(), "wb");
    if (!f || (!first.out.empty() && std::fwrite(first.out.data(), 1, first.out.size(), f) != first.out.size())) return 2;
    std::fclose(f);
    f = std::fopen((prefix + ".members").c_str(), "wb");
    if (!f || (!first.members.empty() && std::fwrite(first.members.data(), sizeof(bl_bgzf_member), first.members.size(), f) != first.members.size())) return 2;
    std::fclose(f);
    const auto& s = first.stats;
    std::printf("%zu %zu %u %u %u %u %u %u %u %u\n", first.out.size(), first.members.size(), s.forms[0], s.forms[1], s.forms[2], s.limited, s.max_len, s.min_len,
                s.max_dist, s.min_dist);
    return 0;
}
