// Drives sampler::hash_sampler over wrapper::kmer_view<__uint128_t, char_iterator> (include/compat/hash_sampler.hpp): the wide view is
// routed to bl_scan_hash_sample128.  tests/test_gpu_superkmer128.py compares the printed values with tests/kmers128_model.py.
//   test_compat_hashsample128 <sequence> <k> <canonical 0|1> <rate> <seed>
// One line per sampled k-mer, "<lo> <hi>", in position order.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "hash_sampler.hpp"

int main(int argc, char** argv)
{
    if (argc != 6) {
        std::fprintf(stderr, "usage: test_compat_hashsample128 <sequence> <k> <canonical 0|1> <rate> <seed>\n");
        return 2;
    }
    try {
        auto view = wrapper::kmer_view_from_cstr<__uint128_t>(argv[1], std::strlen(argv[1]), (uint8_t)std::atoi(argv[2]), std::atoi(argv[3]) != 0);
        using iterator = decltype(view.cbegin());
        sampler::hash_sampler<iterator, hash::hash64> sample(view.cbegin(), view.cend(), hash::hash64(), std::strtoull(argv[5], nullptr, 10), std::atof(argv[4]));
        static_assert(sizeof(decltype(*sample.cbegin())) == 16, "a wide view samples 128-bit values");
        for (auto it = sample.cbegin(); it != sample.cend(); ++it) {
            const unsigned __int128 v = *it;
            std::printf("%llu %llu\n", (unsigned long long)(uint64_t)v, (unsigned long long)(uint64_t)(v >> 64));
        }
    } catch (std::exception const& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    std::printf("test_compat_hashsample128: OK\n");
    return 0;
}
