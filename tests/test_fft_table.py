"""The paired-block schedule table of the frequency-domain engine (csrc/fft.hip, fft_pairs) against the case plan of
tests/test_gpu_fft_table.py — no GPU.  The table is read from the source: a row added, or a kernel pointer removed, without
a case or an UNREACHABLE entry fails here.  And the float64 overlap-save model alone, at every row's block size, stays
within half of the float64 kernels' whole-signal bar on the GPU test's own inputs: each bar is attainable by the method
at that block size before a kernel is blamed."""
import json

import pytest

import _table_probe as tp


@pytest.fixture(scope="module")
def table():
    return tp.parse_table()


@pytest.fixture(scope="module")
def plan(table):
    from soxr_amd import device as dev
    rows, macros = table

    def taps_of(L, M, q):
        p = dev.Plan(*tp.rates_of(L, M), q)     # host only: the plan's design
        assert (p.L, p.M) == (L, M)
        return p.taps

    return tp.case_plan(rows, macros, taps_of)


def test_the_parse_finds_the_table(table):
    rows, macros = table
    assert len(rows) == 46                  # 42 HIPSOXR_PAIR rows and 4 HIPSOXR_PAIR_F32 rows
    assert len({tp.row_key(r) for r in rows}) == len(rows)
    assert macros["HIPSOXR_PAIR"] == list(tp.INSTANCES)
    assert macros["HIPSOXR_PAIR_F32"] == [tp.INSTANCES[0]] + [None] * 9
    assert sum(r["macro"] == "HIPSOXR_PAIR_F32" for r in rows) == 4
    assert sum(len(tp.instances_of(r, macros)) for r in rows) == 42 * 10 + 4


def test_a_changed_table_is_noticed(table):
    """What the parse is for: another row, and a row written out by hand (a pointer turned to nullptr), do not pass."""
    with open(tp.FFT_SRC) as f:
        text = f.read()
    anchor = "HIPSOXR_PAIR(4, 3, 1280, false, 3840, 5120, 384),"
    assert anchor in text
    rows, _ = tp.parse_table(text.replace(anchor, "HIPSOXR_PAIR(5, 3, 1024, false, 3072, 5120, 384), " + anchor))
    assert len(rows) == 47
    with pytest.raises(AssertionError):
        tp.parse_table(text.replace(anchor, "{4, 3, 1280, 0, 384, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr},"))
    _, macros = tp.parse_table(text.replace("k_fft_strided2<PairOf<NA, NB, NT>, double, false>, \\", "nullptr, \\"))
    assert macros["HIPSOXR_PAIR"] != list(tp.INSTANCES)


def test_every_instance_has_a_case_or_a_reason(table, plan):
    rows, macros = table
    cases, status = plan
    assert len(tp.children(rows)) <= 6
    keys = {tp.row_key(r) for r in rows}
    for (row, inst), why in tp.UNREACHABLE.items():
        assert row in keys and "fft_choose_row" in why, (row, inst)
    census = {}
    for r in rows:
        for inst in tp.instances_of(r, macros):
            st = {q: status[(tp.row_key(r), inst, q)] for q in tp.QUALITIES}
            census[(tp.row_key(r), inst)] = st
            if (tp.row_key(r), inst) in tp.UNREACHABLE:
                # listed: then no switch setting reaches it, for either recipe
                assert "case" not in st.values(), (r, inst, st)
            else:
                # not listed: a case for every recipe that admits the row — nothing left out
                assert all(s in ("case", "inadmissible") for s in st.values()), (r, inst, st)
    assert set(tp.UNREACHABLE) <= set(census)
    # every case names its child, and the model sends it to its own row there
    assert len({tp.case_id(c) for c in cases}) == len(cases)
    n_adm = sum(s != "inadmissible" for st in census.values() for s in st.values())
    n_unr = sum(s == "unreachable" for st in census.values() for s in st.values())
    assert len(cases) == n_adm - n_unr
    assert n_unr == 2 * len(tp.UNREACHABLE)
    print(f"{len(cases)} cases, {n_unr} unreachable (instance, recipe) pairs, "
          f"{sum(s == 'inadmissible' for st in census.values() for s in st.values())} inadmissible")


def test_the_design_the_model_uses_is_the_products(table):
    """Taps per phase of the oracle's design == the product's, for every ratio and recipe of the table (the floor fixture
    and the model below are made with the oracle's plan; hop_out follows from the taps)."""
    from soxr_amd import device as dev
    from oracle import oracle as o
    rows, _ = table
    for L, M in sorted({(r["L"], r["M"]) for r in rows}):
        for q in tp.QUALITIES:
            assert o.plan(*tp.rates_of(L, M), q).T == dev.Plan(*tp.rates_of(L, M), q).taps, (L, M, q)


def test_the_method_alone_reaches_the_bars(table, plan, oracle):
    """Reference alone: the float64 overlap-save model at each row's k against the oracle's float64 direct form, on the
    GPU test's inputs — within half of the float64 whole-signal bar (VHQ 2e-9, HQ 1e-6).  The committed fixture holds a
    figure for exactly the admissible (row, recipe) pairs, and today's figures agree with it."""
    from oracle import overlap_save as ovs
    rows, _ = table
    _, status = plan
    with open(tp.FLOOR_JSON) as f:
        floor = json.load(f)["floor"]
    assert set(floor) == {tp.row_name(r) for r in rows}
    for r in rows:
        for q in tp.QUALITIES:
            got = tp.model_floor(oracle, ovs, tp.row_key(r), q)
            adm = status[(tp.row_key(r), ("pair2", "f32"), q)] != "inadmissible"
            have = floor[tp.row_name(r)][q]
            if not adm:
                assert have is None
                continue
            assert got is not None and have is not None, (r, q)
            print(tp.row_name(r), q, got)
            assert got["rel"] <= 0.5 * tp.WHOLE_BAR["f64"][q], (r, q, got)
            for k in ("rel", "stretch", "point"):       # (another FFT library rounds differently: the floor is aliasing, not rounding)
                assert 0.8 * have[k] <= got[k] <= 1.25 * have[k], (r, q, k, got[k], have[k])
