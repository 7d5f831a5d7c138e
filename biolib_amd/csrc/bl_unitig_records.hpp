// bl_unitig_records.hpp — the two records of include/biolib_amd.h that the graph units hand to each other, stated once for the cores
// that read them (bl_links_core.hpp, bl_gfa_core.hpp, bl_steps_core.hpp; bl_clean_core.hpp takes bl_links_core.hpp's).  No HIP: the
// cores compile on the host for tests/emu.  The units that take the public structs from a caller assert the sizes against them.
#pragma once
#include <cstdint>

namespace blrec {

struct alignas(8) Node {  // bl_unitig_node
    uint32_t unitig, rank_flip;
};
struct LinkWords {  // bl_unitig_link: (unitig << 1) | orientation, twice
    uint32_t from, to;
};
static_assert(sizeof(Node) == 8 && sizeof(LinkWords) == 8, "two words each");

}  // namespace blrec
