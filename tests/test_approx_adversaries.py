"""CPU-only: the mined adversaries of tests/golden/approx_adversaries.json (windows on which the approximate hash dword of pass 1 is wrong,
nearly wrong, or must trip a wrap guard) through the CPU emulation of the kernels, record for record against the oracle, planted where
the lane maps make them hard (tests/approx_plant.py), with the redo counters held between two bounds the model gives.

Which kernels decide on murmur64_top in a default build (launch_count_frl / launch_count_mode, mirrored by tests/emu/emu_scan.cpp), all
for canonical 31-mers, w = 11:
  read-tiled, 150 bp (C3)            murmur64_top<true>, guard: a window minimum at prefix 0
  read-tiled, ns = 14 / 15 / 16      the same, read geometry by run time (100, 143 and 286 bp here)
  position-tiled (SY = 2 minimizer)  murmur64_top, guard: st.hmax >= 0xffffffc0 in ANY lane
  C5 closed syncmers (31, 11, {0, 20} and {20, 0})  murmur64_top<true> of 11-mers, undecided below a distance of 2, guard: a dword below 2 in
                                     ANY lane (hlow).  The reference hashes s-mers with seed 0: entries mined there are judged by the oracle
                                     and the model, the wrap entries (seeds 1049, 1103: no 11-mer wraps at seed 0) by the model alone.
The C4 super-k-mer kernel on murmur64_top exists behind BL_SKAX and is not built; the run-time-width closed-syncmer kernels and the
SY = 2 open-offset kernel compare the hashes' own dwords.  None of those reads an approximate dword, so no entry is aimed at them.
The emulation gives lane 63 of a read-tiled wave pad keys for its halo, the device rotates lane 0's keys in: the lanes 62 / 63 placements
meet the device's own halo only in test_gpu_approx_adversaries.py.

Mutations, each applied to a copy of the tree with the emulation rebuilt, and the cases of THIS module that fail under it:
  1.  lane_window_argmin: 128u -> 64u                          test_position_tiled_windows[misordered_one_apart-right]: records differ (the
                                                               window's first unit reported for its last); [one_apart_same_order]: redo count
  1b. lane_window_argmin_frl: dmin < 128u -> 64u               test_read_tiled_windows[L-misordered_one_apart-right]: records differ;
                                                               [L-one_apart_same_order]: redo count; every L
  2.  lane_window_argmin: hmax guard removed                   test_position_tiled_keys[wrap]: records differ; [near_wrap], [wrap_plus_one]: redo count
  3.  hmax guard only in lanes that own windows                test_position_tiled_keys[wrap]: records differ (the key in lane 63 of tile 0's last
                                                               wave); [near_wrap], [wrap_plus_one]: redo count
  4.  lane_window_argmin_frl: `amin < 64u` removed             test_read_tiled_keys[L-wrap_plus_one]: records differ (2988 for 2990 at 143 bp);
                                                               [L-near_wrap], [L-wrap]: redo count; every L
  5.  phase_sync_closed: closest < 2u -> < 1u                  test_closed_syncmers[closed_misordered_hit / _miss / closed_one_apart_same], both
                                                               keys, both offset orders
  5b. phase_sync_closed: `|| low < 2u` (hlow guard) removed    test_closed_syncmers[closed_wrap_plus_one / closed_wrap], both keys, both orders
  6.  read-tiled redo skipped (run_tiles_frl)                  every test_read_tiled_windows and test_read_tiled_keys case
  6c. closed-syncmer redo skipped (run_tiles: `if (any)`)      every test_closed_syncmers case
The suite as it stood before this module (-m "not gpu", all of it, once per mutation; on this tree's sources, i.e. with the emulation's pad
keys already four prefixes apart -- with the old pads the emulation decided every full read-tiled tile twice and could notice less): passes
under 1, 1b, 2, 3, 4, 5 and 5b; under 6 likewise; 6c alone is caught, by test_emu_vs_oracle.py::test_sanitizer_selftest and
::test_golden_units_and_one_mib_digests.  (The nine runs shared one machine: the two-rank gloo tests of test_shard_gloo.py and
test_contig_split.py failed in some of them on their fixed ports, "server socket has failed to listen", whatever the mutation.)
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import approx_plant as P
import hash_top_model as T
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
UNIT, W, SEED = P.UNIT, P.W, P.SEED
WINDOW_CASES, case_entries = P.WINDOW_CASES, P.case_entries


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-s", "-C", EMU_DIR])
    L = C.CDLL(os.path.join(EMU_DIR, "_build", "libbl_emu.so"))
    vp, u64, u = C.c_void_p, C.c_uint64, C.c_uint
    L.emu_batch.restype = vp
    L.emu_batch.argtypes = [vp, u64, vp, u64, u64]
    L.emu_batch_free.argtypes = [vp]
    L.emu_minimizers.argtypes = [vp, u64, u64, u, u, u64, u, vp, vp, vp, u64, vp]
    L.emu_syncmers.argtypes = [vp, u64, u64, u, u, u, u, u64, u, vp, u64, vp]
    L.emu_top_check.argtypes = [vp, u64, u, vp, vp]
    L.emu_top_check_plus_one.argtypes = [vp, u64, u, vp, vp]
    L.emu_top_values.argtypes = [vp, u64, u, C.c_int, vp]
    return L


# ----------------------------------------------------------------------------- the model

def test_model_against_the_hash_and_the_kernels_dwords(emu):
    rng = np.random.default_rng(11)
    for seed in (0, 42, 7, 0xFFFFFFFF):
        keys = rng.integers(0, 2**64, 200_000, dtype=np.uint64)
        keys[:4] = (0, 1, 2**64 - 1, 2**62 - 1)
        h = O.hash64_np(keys, seed)
        assert np.array_equal(T.hash64(keys, seed), h)
        assert np.array_equal(T.true_top(keys, seed), h >> np.uint64(32))  # S + carry IS the hash's high dword
        c = T.carry(keys, seed)
        assert set(np.unique(c)) <= {0, 1} and 0.4 < c.mean() < 0.6
        for plus_one, fn in ((0, T.top), (1, T.top_plus_one)):
            out = np.zeros(len(keys), np.uint32)
            emu.emu_top_values(O._ptr(keys), len(keys), seed, plus_one, O._ptr(out))
            assert np.array_equal(out.astype(np.uint64), fn(keys, seed))
        bad, off = C.c_uint64(), C.c_uint64()
        emu.emu_top_check(O._ptr(keys), len(keys), seed, C.byref(bad), C.byref(off))
        assert bad.value == 0 and off.value == int(c.sum())             # T - S == carry
        emu.emu_top_check_plus_one(O._ptr(keys), len(keys), seed, C.byref(bad), C.byref(off))
        assert bad.value == 0 and off.value == len(keys) - int(c.sum())  # (S + 1) - T == 1 - carry


def test_one_apart_is_misordered_only_on_adjacent_dwords():
    """the bound the kernels rely on, checked on the model: with prefixes one apart the hashes order like the prefixes unless the dwords are
    adjacent with carries (1, 0)"""
    rng = np.random.default_rng(12)
    keys = rng.integers(0, 2**62, 2_000_000, dtype=np.uint64)
    for form in ("top", "top_plus_one"):
        a, h = T.approx(keys, SEED, form), T.hash64(keys, SEED)
        order = np.argsort(a, kind="stable")
        a, h = a[order], h[order]
        lo, hi = slice(0, -1), slice(1, None)
        one = (T.prefix(a[hi]) - T.prefix(a[lo]) == 1) & (a[hi] - a[lo] > 1) & (a[lo] < 0xFFFFFF00) & (a[lo] >= 64)
        assert one.sum() > 1000
        assert (h[hi][one] > h[lo][one]).all()


# ----------------------------------------------------------------------------- the corpus

def test_every_entry_is_what_it_claims():
    seen = set()
    for e in P.corpus():
        form, cls = e["form"], e["class"]
        keys = np.array([int(k, 16) for k in e["keys"]], np.uint64)
        if cls.startswith("closed_"):
            check_closed_entry(e, keys)
            seen.add((form, cls))
            continue
        assert (e["unit"], e["w"], e["seed"], e["canonical"]) == (UNIT, W, SEED, 1)
        seen.add((form, cls))
        assert (keys <= T.revcomp_value(keys, UNIT)).all()  # canonical: the smaller strand
        if cls in P.KEY_CLASSES:
            assert len(e["bases"]) == UNIT and T.units(e["bases"], UNIT, True)[0] == keys[0]
            s, c = int(T.top(keys, SEED)[0]), int(T.carry(keys, SEED)[0])
            if cls == "near_wrap":
                assert T.near_wrap(keys, SEED, form)[0] and not T.wraps(keys, SEED, form)[0] and s != 0xFFFFFFFF
            else:  # S == 0xffffffff exactly: wrapped in the form whose carry it has, at the guarded end without a wrap in the other
                assert s == 0xFFFFFFFF and c == (1 if cls == "wrap" else 0)
                assert T.wraps(keys, SEED, form)[0] == ((cls == "wrap") == (form == "top"))
                assert T.wraps(keys, SEED, form)[0] or T.near_wrap(keys, SEED, form)[0]
                t = int(T.hash64(keys, SEED)[0]) >> 32
                assert t == (0 if cls == "wrap" else 0xFFFFFFFF)  # the smallest / the largest hash dword there is
            continue
        assert len(e["bases"]) == P.SPAN and e["offset"] == 0
        u = T.units(e["bases"], UNIT, True)
        a, h = T.approx(u, SEED, form), T.hash64(u, SEED)
        assert set(int(k) for k in keys) <= set(int(x) for x in u)
        assert not (T.near_wrap(u, SEED, form) | T.wraps(u, SEED, form)).any()
        assert T.must_redo(u, SEED, form, W)[0]
        if cls == "misordered_one_apart":
            assert T.one_apart(a, W)[0] and T.misordered(a, h, W)[0]
            assert int(T.argmin_hash(h, W)[0]) == (0 if e["winner"] == "left" else W - 1)
            sa, sb = sorted(int(x) for x in T.top(keys, SEED))
            assert sb == sa + 1  # adjacent dwords: the only way (see the model)
        elif cls == "one_apart_same_order":
            assert T.one_apart(a, W)[0] and not T.misordered(a, h, W)[0]
        elif cls == "equal_prefix":
            assert T.equal_prefix(a, W)[0] and not T.misordered(a, h, W)[0]
        else:
            raise AssertionError(cls)
    for form in ("top", "top_plus_one"):
        for cls in ("misordered_one_apart", "one_apart_same_order", "equal_prefix") + P.KEY_CLASSES:
            assert (form, cls) in seen
        assert {e["winner"] for e in P.entries(form, ("misordered_one_apart",))} == {"left", "right"}


    for cls in P.CLOSED_CLASSES:
        assert ("top_plus_one", cls) in seen


def check_closed_entry(e, keys):
    cls, seed = e["class"], e["seed"]
    assert (e["unit"], e["w"], e["canonical"], e["form"], len(e["bases"])) == (P.CS, P.CK - P.CS + 1, 1, "top_plus_one", P.CK)
    kmer = e["bases"]
    assert T.units(kmer, P.CK, False)[0] <= T.units(T.revcomp_str(kmer), P.CK, False)[0]  # its own canonical strand
    u = T.units(kmer, P.CS, False)
    assert int(keys[0]) in (int(u[0]), int(u[-1]))  # the key sits at an end of the k-mer
    true_hit, approx_hit, gap, low = T.closed_facts(kmer, P.CS, seed)
    if cls in ("closed_wrap", "closed_wrap_plus_one"):
        assert int(T.top(keys, seed)[0]) == 0xFFFFFFFF and int(T.carry(keys, seed)[0]) == (1 if cls == "closed_wrap" else 0)
        assert low == 0 and approx_hit and true_hit == (cls == "closed_wrap")
        return
    assert seed == 0 and gap == 1 and low >= 2
    sa, sb = sorted(int(x) for x in T.top(keys, seed))
    assert sb == sa + 1
    assert (true_hit, approx_hit) == {"closed_misordered_hit": (True, False), "closed_misordered_miss": (False, True)}.get(cls, (true_hit, true_hit))


# ----------------------------------------------------------------------------- through the emulated kernels

def run(emu, seq, read_len, counter):
    """records of the emulated scan == the oracle's; returns how many tiles the emulation decided a second time"""
    offs = O.fixed_offsets(len(seq), read_len) if read_len else np.array([0, len(seq)], np.uint64)
    v, p, h = O.minimizers(seq, offs, UNIT, W, SEED, True)
    b = emu.emu_batch(O._ptr(seq), len(seq), None, 0, read_len)
    cap = len(seq) + 1
    gv, gp, gh, res = np.zeros(cap, np.uint64), np.zeros(cap, np.uint64), np.zeros(cap, np.uint64), np.zeros(8, np.uint64)
    before = getattr(emu, counter)()
    frl_before = emu.emu_frl_scans()
    emu.emu_minimizers(b, 0, 0, UNIT, W, SEED, 1, O._ptr(gv), O._ptr(gp), O._ptr(gh), cap, O._ptr(res))
    emu.emu_batch_free(b)
    assert (emu.emu_frl_scans() - frl_before == 1) == bool(read_len)  # the layout the case is aimed at
    n = int(res[0])
    assert n == len(v)
    assert np.array_equal(gp[:n], p) and np.array_equal(gv[:n], v) and np.array_equal(gh[:n], h)
    return getattr(emu, counter)() - before


def check_pair(emu, seq, control, read_len, form, counter, planted_tiles):
    must, may = P.redo_bounds(seq, read_len, form)
    assert must >= planted_tiles, "the planted entries are must-redo windows in the tiles they were aimed at"
    redone = run(emu, seq, read_len, counter)
    print(f"read_len {read_len} {form}: redone {redone}, must {sorted(must)}, may {sorted(may)}")
    assert len(must) <= redone <= len(may)
    # the same bases without the plants: the condition is that the model finds nothing a kernel could want to look at twice
    cmust, cmay = P.redo_bounds(control, read_len, form)
    padded = set() if read_len else {(len(control) - 1 - P.POS_ORIGIN) // P.POS_STRIDE}  # (position-tiled: the padding behind the last tile, see redo_bounds)
    assert not cmust and cmay <= padded, "control batch: pick another generator seed (no two keys within a lane's reach with prefixes two or fewer apart, no guard key)"
    assert run(emu, control, read_len, counter) <= len(cmay)
    return redone


@pytest.mark.parametrize("case", WINDOW_CASES)
@pytest.mark.parametrize("L", [150, 100, 143, 286])
def test_read_tiled_windows(emu, L, case):
    g = P.frl_plan(L)
    assert g["ns"] in (14, 15, 16)
    n_reads = 3 * g["reads_per_tile"] + 5
    es = case_entries("top_plus_one", case)
    seq, control = P.frl_batch(es, L, n_reads, seed=1000 + L)
    tiles = {r // g["reads_per_tile"] for (r, _, _) in P.frl_spots(L, n_reads)}
    assert len(tiles) == 4
    check_pair(emu, seq, control, L, "top_plus_one", "emu_frl_redone", tiles)


@pytest.mark.parametrize("cls", P.KEY_CLASSES)
@pytest.mark.parametrize("L", [150, 100, 143, 286])
def test_read_tiled_keys(emu, L, cls):
    """one key per tile.  near_wrap: prefix 0 of murmur64_top<true> without a wrap; wrap_plus_one: dword 0 for a hash dword of 0xffffffff -- left to
    pass 1 it is elected in every window that holds it; wrap: dword 0 and hash dword 0.  143 bp: the read's last lane owns no window, its
    units (tile 2's key among them) are only the halo of the lane before"""
    g = P.frl_plan(L)
    n_reads = (P.FRL_KEY_TILES - 1) * g["reads_per_tile"] + 5
    if L == 143:
        assert g["nwin"] <= (g["lpr"] - 1) * g["ns"]
    es = P.entries("top_plus_one", (cls,))
    assert len(es) == 1
    seq, control = P.frl_batch(es, L, n_reads, seed=2000 + L, keys=True)
    tiles = {r // g["reads_per_tile"] for (r, _) in P.frl_key_spots(L, n_reads)}
    assert len(tiles) == P.FRL_KEY_TILES
    check_pair(emu, seq, control, L, "top_plus_one", "emu_frl_redone", tiles)


N_POS = 2 * P.POS_STRIDE + 1777


@pytest.mark.parametrize("case", WINDOW_CASES)
def test_position_tiled_windows(emu, case):
    es = case_entries("top", case)
    seq, control = P.pos_batch(es, N_POS, seed=3001)
    check_pair(emu, seq, control, 0, "top", "emu_pos_redone", {0, 1, 2})


@pytest.mark.parametrize("cls", P.KEY_CLASSES)
def test_position_tiled_keys(emu, cls):
    """near_wrap: murmur64_top with every prefix bit set; wrap: dword 0xffffffff for a hash dword of 0, the true minimum of every window that
    holds it, which pass 1 would never elect; wrap_plus_one: dword and hash dword 0xffffffff.  One key sits in lane 63 of the last wave of
    tile 0: that lane owns no window, the key is the halo of lane 62's windows there and lane 0's own in tile 1 -- both tiles are decided again"""
    es = P.entries("top", (cls,))
    assert len(es) == 1
    seq, control = P.pos_batch(es, N_POS, seed=3002, keys=True)
    check_pair(emu, seq, control, 0, "top", "emu_pos_redone", {0, 1, 2})


# ----------------------------------------------------------------------------- C5: closed syncmers (31, 11) on murmur64_top<true>

N_CLOSED = 2 * P.CL_STRIDE + 1777


def run_closed(emu, seq, seed, soff, eoff):
    pos = T.closed_syncmers(bytes(seq).decode(), P.CK, P.CS, seed, (soff, eoff))
    n = len(pos)
    if seed == 0:  # the reference's seed: the oracle judges too
        n0, pos0 = O.syncmers(seq, np.array([0, len(seq)], np.uint64), P.CK, P.CS, soff, eoff, True)
        assert n0 == n and np.array_equal(pos0, pos)
    b = emu.emu_batch(O._ptr(seq), len(seq), None, 0, 0)
    got, res = np.zeros(len(seq) + 1, np.uint64), np.zeros(8, np.uint64)
    before, sy2 = emu.emu_closed_redone(), emu.emu_sy2_redone()
    emu.emu_syncmers(b, 0, 0, P.CK, P.CS, soff, eoff, seed, 1, O._ptr(got), len(got), O._ptr(res))
    emu.emu_batch_free(b)
    assert emu.emu_sy2_redone() == sy2  # the closed form, not the argmin form with its exact part deferred
    assert int(res[0]) == n and np.array_equal(got[:n], pos)
    return emu.emu_closed_redone() - before


@pytest.mark.parametrize("offsets", [(0, 20), (20, 0)])
@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("cls", P.CLOSED_CLASSES)
def test_closed_syncmers(emu, cls, which, offsets):
    """every entry (which = 0: the key at the k-mer's first position, 1: at its last) at every spot of closed_spots, against the oracle, for
    both orders of the offsets.  All three tiles hold a comparison the kernel may not trust: each is decided again."""
    e = P.entries("top_plus_one", (cls,), unit=P.CS)[which]
    seq, control = P.closed_batch(e, N_CLOSED, seed=4001)
    pos = T.closed_syncmers(bytes(seq).decode(), P.CK, P.CS, e["seed"], offsets)
    if cls != "closed_one_apart_same":  # the planted k-mers are (not) syncmers as the hashes say, whatever the dwords suggest
        want = T.closed_facts(e["bases"], P.CS, e["seed"])[0]
        assert all((at in set(int(x) for x in pos)) == want for at, _ in P.closed_spots(N_CLOSED))
    redone = run_closed(emu, seq, e["seed"], *offsets)
    print(f"closed {cls}[{which}] {offsets}: redone {redone}")
    assert redone == 3
    assert P.closed_quiet(control, e["seed"]), "control batch: pick another generator seed"
    assert run_closed(emu, control, e["seed"], *offsets) <= 1  # (at most the padding behind the last tile)
