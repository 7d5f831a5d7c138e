// Drives wrapper::kmer_view<__uint128_t, char_iterator> (include/compat/kmer_view.hpp) the way the reference's drivers drive a
// view, and prints what the iteration yields; tests/test_gpu_kmers128.py compares it with tests/golden/kmers128.json.
//   test_compat_kmer128 <sequence> <k> <canonical 0|1> <wide|u64>
// One line per item of the loop `for (it = cbegin(); it != cend(); ++it)`:  "<position> <id> <lo> <hi>"  or  "<position> <id> null",
// then  "last <position> <id> <lo> <hi>"  for the item still readable after the loop (quirk Q1), then the mask as "mask <lo> <hi>".
// u64: the same over kmer_view<uint64_t> (hi is printed as 0), which must keep giving what it gave.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "kmer_view.hpp"

template <typename KmerType>
static void drive(const char* s, std::size_t len, uint8_t k, bool canonical)
{
    auto view = wrapper::kmer_view_from_cstr<KmerType>(s, len, k, canonical);
    auto print = [](const char* tag, wrapper::kmer_context_t<KmerType> const& item) {
        if (!item.value) {
            std::printf("%s%zu %zu null\n", tag, item.position, item.id);
            return;
        }
        const unsigned __int128 v = *item.value;
        std::printf("%s%zu %zu %llu %llu\n", tag, item.position, item.id, (unsigned long long)(uint64_t)v, (unsigned long long)(uint64_t)(v >> 64));
    };
    auto it = view.cbegin();
    for (; it != view.cend(); ++it) print("", *it);
    print("last ", *it);
    const unsigned __int128 mask = it.get_mask();
    std::printf("mask %llu %llu\n", (unsigned long long)(uint64_t)mask, (unsigned long long)(uint64_t)(mask >> 64));
}

int main(int argc, char** argv)
{
    if (argc != 5) {
        std::fprintf(stderr, "usage: test_compat_kmer128 <sequence> <k> <canonical 0|1> <wide|u64>\n");
        return 2;
    }
    static_assert(sizeof(wrapper::kmer_view<__uint128_t, char_iterator>::stored_type) == 16, "128-bit k-mers are stored whole");
    static_assert(sizeof(wrapper::kmer_view<uint64_t, char_iterator>::stored_type) == 8, "64-bit k-mers keep one word");
    // hash::hash64::hash<__uint128_t> on the host is the hash the 128-bit scan returns
    const __uint128_t probe = ((__uint128_t)0x0123456789abcdefULL << 64) | 0xfedcba9876543210ULL;
    if (hash::hash64::hash(probe, 42) != bl_hash64_u128(0xfedcba9876543210ULL, 0x0123456789abcdefULL, 42)) {
        std::fprintf(stderr, "hash64::hash<__uint128_t> differs from bl_hash64_u128\n");
        return 1;
    }
    const uint8_t k = (uint8_t)std::atoi(argv[2]);
    const bool canonical = std::atoi(argv[3]) != 0;
    try {
        if (std::strcmp(argv[4], "wide") == 0) drive<__uint128_t>(argv[1], std::strlen(argv[1]), k, canonical);
        else drive<uint64_t>(argv[1], std::strlen(argv[1]), k, canonical);
    } catch (std::exception const& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    std::printf("test_compat_kmer128: OK\n");
    return 0;
}
