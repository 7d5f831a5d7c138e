"""CPU-only: the self-checks of the cases that drive the count-table family past its grid caps and search depths (scale_cases.py,
select_cases.scale_variants): the cap names are found in the headers, every derived size exceeds its cap, and each batch holds what its
description promises.  The sizes are printed (pytest -s) for the record."""
import numpy as np
import pytest

import read_counts_cases as RC
import read_quantiles_cases as QC
import scale_cases as S
import select_cases as SC


def test_cap_names_are_found_and_sizes_exceed_them():
    cap = S.caps()
    for names in S.CAP_NAMES.values():
        for name in names:
            assert cap[name] >= 1, name
    sizes = S.check_sizes(cap)
    print(sizes)
    assert sizes["scan"]["tiles"] >= cap["TILE_GRID_MAX"] + 4 and sizes["scan"]["reps"] % 2 == 0
    assert sizes["quantiles"]["sequences"] > 4 * cap["WAVE_GRID_MAX"] + 200 or cap["WG_TPB"] != 256


def test_a_retuned_cap_moves_the_sizes_or_fails_by_name():
    """doubling a cap moves the size that exceeds it; a cap far too high fails with a message that names it"""
    cap = S.caps()
    for name in ("TILE_GRID_MAX", "WAVE_GRID_MAX", "WG_GRID_MAX", "INIT_GRID_MAX", "LOOKUP_GRID_MAX", "HIST_LDS_GRID_MAX", "TABLE_GRID_MAX"):
        with pytest.raises(AssertionError, match=name):
            S.check_sizes(dict(cap, **{name: 1 << 26}))
    more = dict(cap, LOOKUP_GRID_MAX=cap["LOOKUP_GRID_MAX"] + 512)
    assert S.query_count(more) > more["LOOKUP_GRID_MAX"] * cap["LTPB"] * cap["G"] and S.check_sizes(more)["table"]["queries"] == S.query_count(more)
    fewer = dict(cap, TILE_GRID_MAX=cap["TILE_GRID_MAX"] // 2)
    assert S.scan_reps(fewer) < S.scan_reps(cap)


@pytest.mark.parametrize("name,k", [("ragged", 31), ("ragged", 33), ("fixed7", 5)])
def test_count_scan_batches(name, k):
    sc = S.scan_case(name, k)
    c = sc["block"]
    if name == "ragged":
        RC.self_check(c)
    assert sc["reps"] % 2 == 0 and S.n_tiles(sc["total"]) >= S.CAPS["TILE_GRID_MAX"] + 4
    assert (np.diff(sc["offs"].astype(np.int64)) >= 0).all() and int(sc["offs"][-1]) == sc["total"] == len(sc["seq"])
    canary = S.canary_record()
    want, (lo, hi) = S.expected_tiled_records(sc, 2, canary)
    assert len(want) == sc["n_seqs"]
    idle = (want.view(np.uint8).reshape(-1, 48) == RC.CANARY_BYTE).all(axis=1)
    if name == "ragged":
        assert (lo, hi) == (1, sc["n_seqs"] - 2) and idle.nonzero()[0].tolist() == [0, sc["n_seqs"] - 1], "the batch's first and last record alone keep the canary"
        per = len(c["offs"]) - 1
        assert RC.same(want[per - 1:per + 1], np.array([RC.IDENTITY, RC.IDENTITY])), "an interior copy's empty first and last record"
        S.three_tile_read_cut(sc)
    else:
        assert (lo, hi) == (0, sc["n_seqs"] - 1) and not idle.any()
        assert sc["n_seqs"] > S.CAPS["INIT_GRID_MAX"] * S.CAPS["ITPB"], "INIT_GRID_MAX: no thread of the identity fill takes a second record"
        assert int(c["offs"][-1] - c["offs"][-2]) == 1, "the last read is one base long"
    counts, valid, words = S.expected_positions(sc)
    assert len(counts) == len(valid) == sc["total"] and words["count"] == int(valid.sum())
    print(name, k, dict(reps=sc["reps"], positions=sc["total"], tiles=S.n_tiles(sc["total"]), sequences=sc["n_seqs"]))


def test_quantile_batch_and_wrong_offsets():
    qc = S.quantile_case()
    print(S.self_check_quantiles(qc))
    b = qc["block"]
    n, n_seqs = len(b["counts"]), len(b["offs"]) - 1
    saw = S.sawtooth_offsets(b)
    alt = S.alternating_offsets(b)
    assert len(saw) == len(alt) == n_seqs + 1 and alt[:4].tolist() == [0, n, 0, n]
    # the model of the property accepts the model's own answers and refuses a row written outside the range
    q, m = QC.expected(b["counts"], b["valid"], b["offs"], 0, n, QC.QUANTILES["ends"])
    written, long_written = S.check_rows_under_wrong_offsets(b, b["offs"], 0, n, QC.QUANTILES["ends"], q, m)
    assert written == n_seqs and long_written == b["forms"].count("workgroup")
    with pytest.raises(AssertionError):
        S.check_rows_under_wrong_offsets(b, alt, 0, n, QC.QUANTILES["ends"], q, m)


def test_table_keys_queries_and_histograms():
    print(S.self_check_tables())
    counts = S.table_counts()
    for nb in S.HIST_BINS:
        want = S.expected_histogram(nb)
        assert int(want.sum()) == len(counts) and len(want) == nb
        for edge in (0, 1, max(nb - 2, 0), nb - 1, nb, S.U32):
            assert (counts == edge).any(), (nb, edge)
    want = S.expected_lookup()
    assert len(want) == S.query_count() and (want != 0).sum() > len(want) // 3


def test_search_depths_and_select_variants():
    depths = SC.scale_depths()
    print(depths)
    assert set(depths.values()) == {0, 1, 2, 3, 4}
    assert [depths[n] for n in (1, 2, 64, 65, 4096, 4097, 262144, 262145)] == [0, 1, 1, 2, 2, 3, 3, 4]
    variants = SC.scale_variants()
    assert {f"depth_{n}" for n in SC.DEPTH_N_OUT} <= set(variants) and {"switch", "switch_first0", "switch_first1", "empty_runs"} <= set(variants)
    assert len([name for name in variants if name.startswith("total_")]) == 10
    for name, v in variants.items():
        m = SC.expected(v)
        inside = SC.scale_self_check(name, v, m)
        if name in ("switch", "empty_runs") or name.startswith("depth_26214"):
            print(name, dict(n_out=m["n_seqs"], n_bases=m["n_bases"], depth=SC.search_depth(m["n_seqs"]), wave_inside=sorted(set(inside.tolist()))[-4:]))
