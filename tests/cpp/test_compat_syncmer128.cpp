// Drives sampler::syncmer_sampler with hash::minimizer_position_extractor over wrapper::kmer_view<__uint128_t, char_iterator>
// (include/compat/syncmer_sampler.hpp, kmer_view.hpp) and prints what it yields; tests/test_gpu_syncmers128.py compares it with
// tests/golden/syncmers128.json.
//   test_compat_syncmer128 <sequence> <k> <s> <start_offset> <end_offset> <canonical 0|1> <wide|u64>
// One line "off <position> <offset>" per k-mer of the loop over the view and for the item still readable after it (quirk Q1): the
// HOST extractor's offset; then per element of the sampler "syn <position> <value>" (the value operator* yields: the k-mer's low
// word for a wide view) and "count <n>" from count().  u64: the same over kmer_view<uint64_t>, which must keep giving what it gave.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "kmer_view.hpp"
#include "syncmer_sampler.hpp"

template <typename KmerType>
static int drive(const char* s, std::size_t len, uint8_t k, uint8_t m, uint16_t so, uint16_t eo, bool canonical)
{
    using view_t = wrapper::kmer_view<KmerType, char_iterator>;
    auto view = wrapper::kmer_view_from_cstr<KmerType>(s, len, k, canonical);
    hash::minimizer_position_extractor ex(k, m);
    auto it = view.cbegin();
    for (; it != view.cend(); ++it) {
        auto item = *it;
        if (item.value) std::printf("off %zu %zu\n", item.position, ex(item));
        else if (ex(item) != (std::size_t)k + 1) return 1;  // a null item: klen + 1
    }
    auto last = *it;
    if (last.value) std::printf("off %zu %zu\n", last.position, ex(last));
    sampler::syncmer_sampler<typename view_t::const_iterator, hash::minimizer_position_extractor> smp(view.cbegin(), view.cend(), ex, so, eo);
    std::size_t n = 0;
    for (auto sit = smp.cbegin(); sit != smp.cend(); ++sit, ++n) {
        const uint64_t value = *sit;
        static_assert(std::is_same<decltype(*sit), uint64_t>::value, "operator* yields PropertyExtractor::value_type");
        if (value != static_cast<uint64_t>(view.values()[sit.position()])) return 1;  // the low word of the k-mer at that position
        std::printf("syn %zu %llu\n", sit.position(), (unsigned long long)value);
    }
    if (n != smp.count() || smp.get_offsets() != std::make_pair(so, eo)) return 1;
    std::printf("count %zu\n", smp.count());
    return 0;
}

int main(int argc, char** argv)
{
    if (argc != 8) {
        std::fprintf(stderr, "usage: test_compat_syncmer128 <sequence> <k> <s> <start_offset> <end_offset> <canonical 0|1> <wide|u64>\n");
        return 2;
    }
    const uint8_t k = (uint8_t)std::atoi(argv[2]), m = (uint8_t)std::atoi(argv[3]);
    const uint16_t so = (uint16_t)std::atoi(argv[4]), eo = (uint16_t)std::atoi(argv[5]);
    const bool canonical = std::atoi(argv[6]) != 0;
    int rc;
    try {
        if (std::strcmp(argv[7], "wide") == 0) rc = drive<__uint128_t>(argv[1], std::strlen(argv[1]), k, m, so, eo, canonical);
        else rc = drive<uint64_t>(argv[1], std::strlen(argv[1]), k, m, so, eo, canonical);
    } catch (std::exception const& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    if (rc != 0) {
        std::fprintf(stderr, "test_compat_syncmer128: inconsistent\n");
        return rc;
    }
    std::printf("test_compat_syncmer128: OK\n");
    return 0;
}
