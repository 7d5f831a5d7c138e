// bl_scan_frl.hpp — the READ-TILED layout of the minimizer / super-k-mer scan for batches of fixed-length short reads
// (plan_scan_frl in bl_scan_core.hpp decides when it applies; 150-bp reads with k = 31, w = 11 is the headline case).
//
// The position-tiled layout (bl_scan_phases.hpp) gives every lane 16 consecutive POSITIONS; on 150-bp reads 30 of every
// 150 positions cannot start a 31-mer, yet they are rolled, hashed and thrown away, and sequence starts are read from a
// 1-bit-per-base vector.  Here a wave takes rpw whole reads, lpr lanes per read, and a lane takes NS consecutive UNIT
// STARTS of its read (150 bp, k = 31: 8 reads per wave, 8 lanes per read, 15 units per lane = all 120 units of a read):
//   * the unit-1 tail positions of a read are never hashed (1.27 x fewer hashes per useful window at C3),
//   * reads do not share windows, so a wave needs no halo from the next wave tile,
//   * where a read starts and which windows exist is arithmetic on (lane, slot): no start_bits, no flag gathering,
//   * bases that are not ACGTUacgtu are the only thing left to look up, and only in tiles that hold one.
// Semantics are those of the position-tiled scan (reference minimizer_view.hpp:229-245: the window is cleared at a break
// and at a sequence end; leftmost minimum wins, :283,374) and the record order is the same, so both layouts produce
// identical arrays; tests/emu runs these phases thread by thread against the oracle under ASan.
#pragma once
#include "bl_scan_phases.hpp"

namespace bl {

// global position the tile's staged chunk 0 starts at (both layouts)
BL_DEV int64_t tile_q0(const ScanParams& p, uint32_t tile)
{
    const int64_t g = p.origin + (int64_t)tile * p.stride;
    return p.frl ? (g & ~15LL) : g;  // read-tiled: origin >= 0, tiles start at a read, not at a 16-byte boundary
}

// ------------------------------------------------------------------------------------------------
// Phase 1: coalesced 16-byte loads -> 2-bit codes + good-base bits; true if the chunk holds a break
template <bool PACKED = false>  // as stage_chunk
BL_DEV bool stage_chunk_frl(const ScanParams& p, uint32_t* codes, uint32_t* flags, int c, int64_t q0)
{
    const int64_t g = q0 + 16 * (int64_t)c;  // >= 0, a multiple of 16 (tile_q0)
    uint32_t code = 0, bad = 0;
    bool ascii = true;
    if (PACKED) {
        const bool pbad = packed_chunk(p, g, code);
        ascii = BL_COLD(wave_any(pbad));
    }
    if (ascii) {  // no packed copy, or a lane of the wave meets a break or the end of the batch
        uint32_t d[4] = {0, 0, 0, 0};
        if (g + 16 <= p.n_bases) {
            const Vec16 v = *reinterpret_cast<const Vec16*>(p.bases + g);
            d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        } else if (BL_COLD(g < p.n_bases)) {  // ragged end of the batch: byte-wise, zeros (= breaks) outside
            for (int b = 0; b < 16; ++b) {
                const int64_t q = g + b;
                if (q < p.n_bases) d[b >> 2] |= (uint32_t)p.bases[q] << (8 * (b & 3));
            }
        }
        encode16(d, code, bad);
    }
    codes[c] = code;
    flags[c] = ~bad & 0xffffu;
    return bad != 0;
}

template <int MODE, int W, bool PACKED = false>
BL_DEV void phase_load_frl(const ScanParams& p, TileShared<MODE, W>& sh, int tid, int64_t q0)
{
    bool bad = false;
    for (int c = tid; c < p.slot_chunks; c += TPB) bad |= stage_chunk_frl<PACKED>(p, sh.codes, sh.flags, c, q0);  // 2 rounds at most; the 2nd is a few lanes of wave 0
    const int wv = wave_index(tid);
#if defined(__HIP_DEVICE_COMPILE__) && !defined(BL_CPU_EMU)
    const bool any = wave_any(bad);
    if ((tid & 63) == 0) sh.wave_bad[wv] = any ? 1u : 0u;
#else
    if ((tid & 63) == 0) sh.wave_bad[wv] = 0;  // threads of a wave are emulated in order
    if (bad) sh.wave_bad[wv] = 1;
#endif
}

// A tile of a PACKED scan whose staged chunks [q0 >> 4, (q0 >> 4) + slot_chunks) are all good ones needs no staging: what phase_load_frl
// would put into sh.codes is, bit for bit, codes_packed from q0 >> 4 on, and nobody looks at sh.flags.  The test ORs whole words of
// chunk_bad, those that hold a bit of a staged chunk and no others (packed_covers promises the staged chunks, guards included, not their
// neighbours' words): a bad chunk of a neighbouring tile in one of them costs a staging that was not needed, nothing else.  q0, and so
// every address, is the same for the whole workgroup: scalar loads on the device, nmin or nmin + 1 of them (10 or 11 for 150-bp reads).
BL_DEV bool frl_tile_clean(const ScanParams& p, int64_t q0)
{
    const int64_t c0 = q0 >> 4;  // q0 >= 0 (tile_q0)
    const uint32_t* wp = p.chunk_bad + (c0 >> 5);
    const int nmin = (p.slot_chunks + 31) >> 5, nw = (int)(((c0 & 31) + p.slot_chunks + 31) >> 5);  // nw - nmin is 0 or 1
    uint32_t any = 0;
    for (int i = 0; i < nmin; ++i) any |= wp[i];
    if (nw > nmin) any |= wp[nmin];
    return any == 0;
}

// four consecutive dwords of the packed copy, at any dword (one global_load_dwordx4)
#if defined(__HIP_DEVICE_COMPILE__) && !defined(BL_CPU_EMU)
typedef uint32_t PackedQuad __attribute__((ext_vector_type(4), aligned(4)));
#endif
BL_DEV void load_packed4(const uint32_t* q, uint32_t& c0, uint32_t& c1, uint32_t& c2, uint32_t& c3)
{
#if defined(__HIP_DEVICE_COMPILE__) && !defined(BL_CPU_EMU)
    const PackedQuad v = *reinterpret_cast<const PackedQuad*>(q);
    c0 = v.x; c1 = v.y; c2 = v.z; c3 = v.w;
#else
    c0 = q[0]; c1 = q[1]; c2 = q[2]; c3 = q[3];
#endif
}

// ------------------------------------------------------------------------------------------------
// Phase 2: which read and which units this lane owns; roll and hash them.
// GENERIC: run-time unit length (see phase_hash: those kernels hash with the compiler's own multiply)
// APPROX: st.h[s] holds murmur64_top<true> (S + 1) in its high dword (low dword 0): the window phase works on those and reports what it
// cannot decide (lane_window_argmin_frl)

// The 64 bits of codes that END at base e (0 <= e < 48) of the 48 bases a0:a1:a2 (first base in the top pair of a0): bases e - 31 .. e,
// the last one in the low pair.  Bases before 0 read as zeros.  Ending rather than starting at a base keeps every shift of v_alignbit_b32
// inside 0..30 (a 64-bit window that starts on a word boundary would need a shift of 32, which the instruction takes modulo 32).
BL_DEV uint64_t bases_ending_at(uint32_t a0, uint32_t a1, uint32_t a2, int e)
{
    const int q = e >> 4, sh = 30 - 2 * (e & 15);
    const uint32_t w[3] = {a0, a1, a2};
    const uint32_t lo = sh == 0 ? w[q] : (q == 0 ? w[0] >> sh : funnel_shr(w[q - 1], w[q], sh));
    const uint32_t hi = q == 0 ? 0u : (sh == 0 ? w[q - 1] : (q == 1 ? w[0] >> sh : funnel_shr(w[q - 2], w[q - 1], sh)));
    return ((uint64_t)hi << 32) | lo;
}

// Units of length U (16 < U <= 32, a compile-time constant) by direct extraction: unit s is the U bases that end at base s + U - 1 of
// the lane's 48, its reverse complement the U bases that end at base 47 - s of their reverse complement (three revcomp16 per lane, for
// NS units): two v_alignbit_b32 and a mask per strand, where the rolling registers (Roller) cost 8 instructions per unit.
template <int U>
BL_DEV void units_direct(uint32_t a0, uint32_t a1, uint32_t a2, uint32_t r0, uint32_t r1, uint32_t r2, int s, uint64_t& fw, uint64_t& rv)
{
    static_assert(U > 16 && U <= 32, "direct extraction: 16 < U <= 32");
    constexpr uint64_t M = U == 32 ? ~0ull : (1ull << (2 * U)) - 1;
    fw = bases_ending_at(a0, a1, a2, s + U - 1) & M;
    rv = bases_ending_at(r0, r1, r2, 47 - s) & M;
}

// U: the unit length where the kernel fixes it (0: from p.unit).  31 (the C3 shape) with NS <= 17 takes the units by direct
// extraction (units_direct); every other length keeps the rolling registers.  In the CPU emulation U is 0 and p.unit decides.
// tile_codes: where the tile's chunk 0 lies in the packed copy, for a tile that was not staged (frl_tile_clean); nullptr: sh.codes holds it
template <int MODE, int W, int NS, bool GENERIC = false, bool APPROX = false, int U = 0>
BL_DEV void phase_hash_frl(const ScanParams& p, TileShared<MODE, W>& sh, int tid, int64_t q0, uint32_t tile, ThreadState& st, const uint32_t* tile_codes = nullptr)
{
    const int wv = wave_index(tid), lane = tid & 63;
    const int r = (int)(((uint32_t)lane * p.lpr_inv) >> 16);  // read of this wave the lane works on
    const int j = lane - r * p.lpr;                           // lane inside that read
    const int64_t read_idx = ((int64_t)tile * NWAVE + wv) * p.rpw + r;
    const bool active = r < p.rpw && read_idx < p.n_reads;
    const int off0 = (int)(p.origin + (int64_t)tile * p.stride - q0);  // 0..15
    const int base = active ? off0 + (wv * p.rpw + r) * p.read_len + j * NS : off0;
    st.lane_base = base;
    st.jlane = active ? j : -1;
    // the lane's 48 bases from `base` on: four dwords, staged ones or the packed copy's own, funnel-shifted to the lane's own alignment
    // (two loads in two branches: one load through a pointer chosen between LDS and HBM would be a flat load)
    uint32_t c0, c1, c2, c3;
    if (tile_codes) {
        load_packed4(tile_codes + (base >> 4), c0, c1, c2, c3);
    } else {
        const uint32_t* cp = sh.codes + (base >> 4);
        c0 = cp[0]; c1 = cp[1]; c2 = cp[2]; c3 = cp[3];
    }
    const int sh2 = 2 * (base & 15);
    const uint32_t a0 = (uint32_t)(((((uint64_t)c0 << 32) | c1) << sh2) >> 32);
    const uint32_t a1 = (uint32_t)(((((uint64_t)c1 << 32) | c2) << sh2) >> 32);
    const uint32_t a2 = (uint32_t)(((((uint64_t)c2 << 32) | c3) << sh2) >> 32);
    constexpr bool DIRECT_OK = !GENERIC && (U == 0 || U == 31) && NS + 31 - 1 <= 47;
    if (DIRECT_OK && (U == 31 || p.unit == 31)) {
        const uint32_t r0 = revcomp16(a2), r1 = revcomp16(a1), r2 = revcomp16(a0);
        BL_UNROLL
        for (int s = 0; s < NS; ++s) {
            uint64_t fw, rv;
            units_direct<31>(a0, a1, a2, r0, r1, r2, s, fw, rv);
            const uint64_t v = p.canonical ? min62<31>(rv, fw) : fw;  // minimizer_view.hpp:236-238
            st.h[s] = APPROX ? (uint64_t)murmur64_top<true>(v, p.seed) << 32 : murmur64(v, p.seed);
        }
        return;
    }
    Roller rr;
    roller_start(rr, a0, a1, a2, p.unit);
    BL_UNROLL
    for (int s = 0; s < NS; ++s) {
        roller_step(rr, s);
        const uint64_t fw = roller_fwd(rr), rv = roller_rc(rr);
        const uint64_t v = (p.canonical && rv < fw) ? rv : fw;  // minimizer_view.hpp:236-238
        if (APPROX) st.h[s] = (uint64_t)murmur64_top<true>(v, p.seed) << 32;
        else st.h[s] = GENERIC ? murmur64_plain(v, p.seed) : murmur64(v, p.seed);
    }
}

// ------------------------------------------------------------------------------------------------
// Neighbouring lanes: values of lane - 1 / lane + 1 (DPP wave shifts on the GPU, lane 0 / 63 get their own value back,
// which no owned window ever uses; the emulation reads the neighbour's state).
#if defined(__HIP_DEVICE_COMPILE__) && !defined(BL_CPU_EMU)
BL_DEV uint32_t dpp_next32(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x130, 0xf, 0xf, true); }  // wave_shl:1
// the same as a rotation: lane 63 reads lane 0 (wave_rol:1)
BL_DEV uint32_t dpp_next32_rot(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x134, 0xf, 0xf, true); }
BL_DEV uint32_t dpp_prev32(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x138, 0xf, 0xf, true); }  // wave_shr:1
// dpp_next32_rot(v) + k as ONE v_add_u32_dpp (the builtin and an add compile to v_mov_b32_dpp + v_add_u32).  A DPP operand written by the
// VALU instruction just before needs two wait states, and the assembler does not look inside the asm: hence the s_nop.
BL_DEV uint32_t dpp_next32_rot_add(uint32_t v, uint32_t k)
{
    uint32_t d;
    asm("s_nop 1\n\tv_add_u32_dpp %0, %1, %2 wave_rol:1 row_mask:0xf bank_mask:0xf" : "=v"(d) : "v"(v), "v"(k));
    return d;
}
#endif

// Window argmins of a lane that owns NS elements: the W - 1 halo elements come from the following lanes, NS per hop.
// a[i] = raw packed key (element index in its low 6 bits) or, after the exact branch, the plain element index.
// APPROX (keys from murmur64_top<true>): no exact form in here; *tie is set when a lane that owns windows met two keys less than two
// prefixes apart, or one of its windows has its minimum at prefix 0 (a key that may have wrapped), and the caller has the whole tile
// decided again (scan_redo_frl_kernel)
template <int NS, int W, bool APPROX = false>
BL_DEV void lane_window_argmin_frl(const ThreadState* all, int tid, const ThreadState& st, bool owns, uint32_t* a, bool* tie = nullptr)
{
    constexpr int NE = W - 1, NK = NS + NE;  // NK <= 64: 6-bit tags
    uint32_t key[NK];
    BL_UNROLL
    for (int s = 0; s < NS; ++s) key[s] = packed_key((uint32_t)(st.h[s] >> 32), s, true);
#if defined(__HIP_DEVICE_COMPILE__) && !defined(BL_CPU_EMU)
    (void)all;
    (void)tid;
    if constexpr (APPROX && NE <= NS) {  // one hop: the halo is the next lane's first W - 1 keys, their tags moved on by NS in the same instruction
        const uint32_t ns = (uint32_t)NS;
        BL_UNROLL
        for (int x = 0; x < NE; ++x) key[NS + x] = dpp_next32_rot_add(key[x], ns);
    } else {
        uint32_t cur[NS];
        BL_UNROLL
        for (int x = 0; x < NS; ++x) cur[x] = key[x];
        BL_UNROLL
        for (int hop = 0; hop * NS < NE; ++hop) {
            BL_UNROLL
            for (int x = 0; x < NS; ++x) {
                // lane 63 owns windows too (64 = rpw * lpr lanes at work) but has no lane to take a halo from: the shift is a ROTATION
                // and it gets lane 0's keys — some other read's, as good as random — so that its (non-existent) halo windows look
                // like a hash tie no more often than real ones; what they choose is cleared (phase_window_frl_a).  (A rotation reads
                // a lane everywhere: no `old` operand to initialise, one v_mov per element less than a shift with pad keys.)
                if (hop * NS + x < NE || (hop + 1) * NS + x < NE || (hop + 2) * NS + x < NE)
                    cur[x] = dpp_next32_rot(cur[x]) + (uint32_t)NS;
                if (hop * NS + x < NE) key[(hop + 1) * NS + x] = cur[x];
            }
        }
    }
#else
    {
        const int lane = tid & 63;
        for (int x = 0; x < NE; ++x) {
            const int nb = lane + 1 + x / NS;
            const uint32_t hi = nb < 64 ? (uint32_t)(all[tid + 1 + x / NS].h[x % NS] >> 32) : (0x03fffff0u - 4u * (uint32_t)x) << 6;  // pads, four prefixes apart: no tie among themselves, on hashes (< 64) or on murmur64_top (< 128, tags included)
            key[NS + x] = packed_key(hi, NS + x, true);
        }
    }
#endif
    const uint32_t dmin = window_argmin_packed<NS, W, true, true, APPROX>(key, a);
    if (APPROX) {
        // The keys hold S' = murmur64_top<true> = S + 1, and the hash's high dword T is S' or S' - 1.  Without a wrap, prefixes two or more
        // apart order keys like their hashes (dmin, above).  The one value that can wrap is S' = 0 (T = 0xffffffff): such a key looks like
        // the smallest there is while its hash is the largest.  It can only mislead a window it is the minimum of: a window that holds a
        // key of prefix 0 has a minimum of prefix 0 (nothing packs below it), be it that key or another one.  So a tile is decided again
        // when some window a lane owns has its minimum at prefix 0, and every window that holds a wrapped key is among those.  One
        // v_min3_u32 finds the smallest minimum of the lane's windows: windows 0, W, 2W, ... and NS - 1 cover all of its keys.  (With
        // murmur64_top itself the value that can wrap is the LARGEST, which may sit in any window: that took a running maximum of every
        // hash, 15 v_max_u32 per lane.)
        uint32_t amin = a[NS - 1];
        BL_UNROLL
        for (int s = 0; s < NS - 1; s += W) amin = a[s] < amin ? a[s] : amin;
        if (owns && (dmin < 128u || amin < 64u)) *tie = true;
        return;
    }
    if (BL_COLD(wave_any(owns && dmin < 64u))) {  // a prefix tie somewhere in the wave: the exact 64-bit form
        uint64_t e[NK];
        BL_UNROLL
        for (int s = 0; s < NS; ++s) e[s] = st.h[s];
#if defined(__HIP_DEVICE_COMPILE__) && !defined(BL_CPU_EMU)
        uint64_t cur[NS];
        BL_UNROLL
        for (int x = 0; x < NS; ++x) cur[x] = st.h[x];
        BL_UNROLL
        for (int hop = 0; hop * NS < NE; ++hop) {
            BL_UNROLL
            for (int x = 0; x < NS; ++x) {
                if (hop * NS + x < NE || (hop + 1) * NS + x < NE || (hop + 2) * NS + x < NE) cur[x] = lane_next(cur[x]);
                if (hop * NS + x < NE) e[(hop + 1) * NS + x] = cur[x];
            }
        }
#else
        const int lane = tid & 63;
        for (int x = 0; x < NE; ++x) {
            const int nb = lane + 1 + x / NS;
            e[NS + x] = nb < 64 ? all[tid + 1 + x / NS].h[x % NS] : 0xDEADBEEFDEADBEEFull;
        }
#endif
        window_argmin<NS, W, true>(e, a);
    }
}

// bit s: every base of the window that starts at staged position base + s, span bases long, is one of ACGTUacgtu
// (only run for tiles that hold a break)
template <int NS>
BL_DEV uint32_t frl_good_mask(const ScanParams& p, const uint32_t* flags, int base, int span)
{
    const int ch = base >> 4, off = base & 15;
    uint64_t g[3] = {0, 0, 0};
    for (int c = 0; c < 9; ++c) {  // 144 staged bits cover off + 15 + 95 positions
        int idx = ch + c;
        idx = idx < p.slot_chunks ? idx : p.slot_chunks - 1;  // beyond the staged tile: only windows that do not exist look there
        g[c >> 2] |= (uint64_t)(flags[idx] & 0xffffu) << (16 * (c & 3));
    }
    Bits128 good;
    good.lo = off ? (g[0] >> off) | (g[1] << (64 - off)) : g[0];
    good.hi = off ? (g[1] >> off) | (g[2] << (64 - off)) : g[1];
    return (uint32_t)and_run(good, span).lo & ((1u << NS) - 1);
}

// ------------------------------------------------------------------------------------------------
// ELEMENT-CENTRIC decisions (minimizer scans).  A minimizer occurrence is one ELEMENT (unit start) that is the argmin of at
// least one valid window: the valid windows that choose an element are consecutive (leftmost minimum: if windows i < j
// choose e, every window between them lies inside their union and chooses e too, and it is valid because its bases are
// theirs), and argmins never move left as the window slides, so the records of a scan — "one each time the occurrence
// changes or a run starts", minimizer_view.hpp:193-208 — are exactly the chosen elements in position order.  A lane
// therefore ORs one bit per window into a mask indexed by element (v_lshl_or_b32: the element index is the low bits of the
// packed minimum), hands the bits of elements >= NS to the lane that owns them (one DPP move: valid windows never leave
// the read, W - 1 <= NS) and lists its own set bits.  No per-window comparison with the previous window, no byte-packed
// argmins, no start/end masks.  Applies when the mask fits a dword.
template <int MODE, int W, int NS>
constexpr bool frl_occ_form() { return MODE == MODE_MINIMIZER && W > 1 && W - 1 <= NS && NS + W - 1 <= 32; }

// Phase 3a: window argmins of the lane's NS windows and which of them exist.
// LIM_LAST != 0 (the compile-time geometry of scan_count_frl_kernel): every lane of a read owns NS windows but the last,
// which owns LIM_LAST (1..NS); 0: any geometry.
// clean: the tile was not staged (frl_tile_clean: no break in it, and sh.wave_bad and sh.flags hold nothing of this tile)
template <int MODE, int W, int NS, int LIM_LAST = 0, bool APPROX = false>
BL_DEV void phase_window_frl_a(const ScanParams& p, TileShared<MODE, W>& sh, int tid, ThreadState& st, const ThreadState* all, bool* tie = nullptr, bool clean = false)
{
    uint32_t a[S];
    lane_window_argmin_frl<NS, (W > 1 ? W : 2), APPROX>(all, tid, st, st.jlane >= 0, a, tie);
    // windows of the read: window index j * NS + s must be below nwin; breaks only where the tile holds one
    uint32_t vmask = 0;
    if (st.jlane >= 0) {
        int lim = p.nwin - st.jlane * NS;
        lim = lim < 0 ? 0 : (lim > NS ? NS : lim);
        vmask = (1u << lim) - 1u;
    }
    const uint32_t tile_bad = clean ? 0u : sh.wave_bad[0] | sh.wave_bad[1] | sh.wave_bad[2] | sh.wave_bad[3];
    if (BL_COLD(tile_bad)) vmask &= frl_good_mask<NS>(p, sh.flags, st.lane_base, p.unit + (W > 0 ? W : p.w) - 1);
    st.vmask = vmask;
    if (frl_occ_form<MODE, W, NS>()) {
        uint32_t occ = 0;
        if (LIM_LAST == 0 || BL_COLD(tile_bad)) {
            BL_UNROLL
            for (int s = 0; s < NS; ++s) occ |= ((vmask >> s) & 1u) << (a[s] & 31u);
        } else {
            BL_UNROLL
            for (int s = 0; s < NS; ++s) occ |= 1u << (a[s] & 31u);
            // windows that do not exist (the read's last lane) set bits too, none below the argmin of the last window
            // that does (argmins never move left): clear everything above it
            const uint32_t a_sel = st.jlane == p.lpr - 1 ? a[LIM_LAST > 0 ? LIM_LAST - 1 : 0] : a[NS - 1];
            occ &= (2u << (a_sel & 31u)) - 1u;
            if (st.jlane < 0) occ = 0;
        }
        st.occ = occ;
        return;
    }
    BL_UNROLL
    for (int s = NS; s < S; ++s) a[s] = 0;
    uint32_t apk[4];
    BL_UNROLL
    for (int q = 0; q < 4; ++q) {  // byte s of apk = element index of the argmin of window s
        const uint32_t lo2 = byte_perm(a[4 * q + 1], a[4 * q], 0x0c0c0400u);
        const uint32_t hi2 = byte_perm(a[4 * q + 3], a[4 * q + 2], 0x04000c0cu);
        apk[q] = (lo2 | hi2) & 0x3f3f3f3fu;
    }
    st.apk0 = ((uint64_t)apk[1] << 32) | apk[0];
    st.apk1 = ((uint64_t)apk[3] << 32) | apk[2];
    st.a_first = a[0] & 63u;
    st.a_last = a[NS - 1] & 63u;
}

// Phase 3b: start / end decisions.  Returns starts | ends << 16.
template <int MODE, int W, int NS>
BL_DEV uint32_t phase_window_frl_b(const ScanParams& p, int tid, ThreadState& st, const ThreadState* all)
{
    if (frl_occ_form<MODE, W, NS>()) {  // take over the bits the previous lane found for this lane's elements
#if defined(__HIP_DEVICE_COMPILE__) && !defined(BL_CPU_EMU)
        (void)all;
        (void)tid;
        const uint32_t prev = dpp_prev32(st.occ);
#else
        const uint32_t prev = (tid & 63) > 0 ? all[tid - 1].occ : 0u;
#endif
        st.endm = 0;
        st.emit = (st.occ | (prev >> NS)) & ((1u << NS) - 1u);
        return (uint32_t)__builtin_popcount(st.emit);
    }
#if defined(__HIP_DEVICE_COMPILE__) && !defined(BL_CPU_EMU)
    (void)all;
    (void)tid;
    const uint32_t prev_last = dpp_prev32(st.a_last), prev_vm = dpp_prev32(st.vmask);
    const uint32_t next_first = dpp_next32(st.a_first), next_vm = dpp_next32(st.vmask);
#else
    const int lane = tid & 63;
    const uint32_t prev_last = lane > 0 ? all[tid - 1].a_last : 0xAAu, prev_vm = lane > 0 ? all[tid - 1].vmask : 0xAAAAu;
    const uint32_t next_first = lane < 63 ? all[tid + 1].a_first : 0x55u, next_vm = lane < 63 ? all[tid + 1].vmask : 0x5555u;
#endif
    const int j = st.jlane;
    const uint32_t apk[4] = {(uint32_t)st.apk0, (uint32_t)(st.apk0 >> 32), (uint32_t)st.apk1, (uint32_t)(st.apk1 >> 32)};
    // differ bit s: the argmin of window s is another occurrence than that of window s - 1 (the previous lane's last
    // window for s = 0: its element index moves by NS into this lane's frame; an index below NS there wraps to >= 112)
    const uint32_t p0 = (prev_last - (uint32_t)NS) & 0x7fu;
    uint32_t differ = 0;
    BL_UNROLL
    for (int q = 0; q < 4; ++q) {
        const uint32_t prv = q ? funnel_shr(apk[q], apk[q - 1], 24) : ((apk[0] << 8) | p0);
        const uint32_t x = apk[q] ^ prv;                             // bytes < 128
        const uint32_t nz = ((x + 0x7f7f7f7fu) >> 7) & 0x01010101u;  // 1 in every non-zero byte
        differ |= ((nz * 0x01020408u) >> 24) << (4 * q);             // byte b -> bit b
    }
    const uint32_t vm = st.vmask;
    const uint32_t pv = (j > 0) ? ((prev_vm >> (NS - 1)) & 1u) : 0u;  // the window before this lane's first, same read
    const uint32_t vprev = (vm << 1) | pv;
    st.emit = vm & (~vprev | differ);  // window s starts an occurrence
    st.endm = 0;
    if (MODE == MODE_SUPERKMER) {
        const uint32_t nv = (j >= 0 && j < p.lpr - 1) ? (next_vm & 1u) : 0u;  // the window after this lane's last, same read
        const uint32_t dn = ((next_first + (uint32_t)NS) != st.a_last) ? 1u : 0u;
        const uint32_t vnext = (vm >> 1) | (nv << (NS - 1));
        const uint32_t dnext = (differ >> 1) | (dn << (NS - 1));
        st.endm = vm & (~vnext | dnext);  // window s ends one
    }
    return (uint32_t)__builtin_popcount(st.emit) | ((uint32_t)__builtin_popcount(st.endm) << 16);
}

// ------------------------------------------------------------------------------------------------
// Phase 4: tile-local compaction.  List entries are FLAT positions relative to the tile's first staged chunk
// (< 16 * NCHUNK), not (wave, wave-relative position) pairs: pass 2 tells the two apart by p.frl.
template <int MODE, int W, int NS = 0>
BL_DEV void phase_list_frl(TileShared<MODE, W>& sh, const ThreadState& st, uint32_t excl_s, uint32_t excl_e)
{
    uint32_t m = st.emit;
    uint32_t r = excl_s;
    if (NS != 0 && frl_occ_form<MODE, W, (NS ? NS : 1)>()) {  // bit s: the lane's own element s is a minimizer occurrence
        while (m) {
            const int s = __builtin_ctz(m);
            m &= m - 1;
            sh.list_a[r] = (uint16_t)(st.lane_base + s);
            ++r;
        }
        return;
    }
    while (m) {
        const int s = __builtin_ctz(m);
        m &= m - 1;
        const uint32_t arel = (uint32_t)((s < 8 ? st.apk0 : st.apk1) >> (8 * (s & 7))) & 0xffu;
        sh.list_a[r] = (uint16_t)((uint32_t)st.lane_base + arel);
        if (MODE == MODE_SUPERKMER) sh.list_j[r] = (uint16_t)(st.lane_base + s);
        ++r;
    }
    if (MODE == MODE_SUPERKMER) {
        m = st.endm;
        r = excl_e;
        while (m) {
            const int s = __builtin_ctz(m);
            m &= m - 1;
            sh.list_e[r] = (uint16_t)(st.lane_base + s);
            ++r;
        }
    }
}

}  // namespace bl
