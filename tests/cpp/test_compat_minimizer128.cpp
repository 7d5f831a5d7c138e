// Drives sampler::minimizer_sampler with hash::hash64 over wrapper::kmer_view<__uint128_t, char_iterator>
// (include/compat/minimizer_sampler.hpp, kmer_view.hpp) and prints what it yields; tests/test_gpu_minimizers128.py compares it with
// the Python model (tests/minimizers128_model.py).
//   test_compat_minimizer128 <sequence> <k> <w> <canonical 0|1> <wide|u64>
// Per element of the sampler "min <position> <low word> <high word>" (position = id; the value operator* yields), then "count <n>".
// u64: the same over kmer_view<uint64_t>, which must keep giving what it gave (the high word printed is 0).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "kmer_view.hpp"
#include "minimizer_sampler.hpp"

template <typename KmerType>
static int drive(const char* s, std::size_t len, uint8_t k, uint16_t w, bool canonical)
{
    using view_t = wrapper::kmer_view<KmerType, char_iterator>;
    auto view = wrapper::kmer_view_from_cstr<KmerType>(s, len, k, canonical);
    sampler::minimizer_sampler<typename view_t::const_iterator, hash::hash64> smp(view.cbegin(), view.cend(), hash::hash64(), 0, w);
    if (smp.get_w() != w) return 1;
    std::size_t n = 0;
    for (auto it = smp.cbegin(); it != smp.cend(); ++it, ++n) {
        auto const& item = *it;
        static_assert(std::is_same<std::decay_t<decltype(*item.value)>, KmerType>::value, "operator* yields the view's kmer_context_t");
        if (!item.value || item.position != item.id) return 1;
        if (*item.value != static_cast<KmerType>(view.values()[item.position])) return 1;  // the k-mer at that position, all its bits
        const __uint128_t v = *item.value;
        std::printf("min %zu %llu %llu\n", item.position, (unsigned long long)(uint64_t)v, (unsigned long long)(uint64_t)(v >> 64));
    }
    std::printf("count %zu\n", n);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc != 6) {
        std::fprintf(stderr, "usage: test_compat_minimizer128 <sequence> <k> <w> <canonical 0|1> <wide|u64>\n");
        return 2;
    }
    const uint8_t k = (uint8_t)std::atoi(argv[2]);
    const uint16_t w = (uint16_t)std::atoi(argv[3]);
    const bool canonical = std::atoi(argv[4]) != 0;
    int rc;
    try {
        if (std::strcmp(argv[5], "wide") == 0) rc = drive<__uint128_t>(argv[1], std::strlen(argv[1]), k, w, canonical);
        else rc = drive<uint64_t>(argv[1], std::strlen(argv[1]), k, w, canonical);
    } catch (std::exception const& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    if (rc != 0) {
        std::fprintf(stderr, "test_compat_minimizer128: inconsistent\n");
        return rc;
    }
    std::printf("test_compat_minimizer128: OK\n");
    return 0;
}
