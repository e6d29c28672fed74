"""The paired-block schedule table of the frequency-domain engine (csrc/fft.hip, fft_pairs) against the case plan of
tests/test_gpu_fft_table.py — no GPU.  The table is read from the source: a row added, or a kernel pointer removed, without
a case or an UNREACHABLE entry fails here.  And the float64 overlap-save model alone, at every row's block size, stays
within half of the float64 kernels' whole-signal bar on the GPU test's own inputs: each bar is attainable by the method
at that block size before a kernel is blamed.  The float16 / bfloat16 table (fft_half_kernels) likewise, against the case
plan of tests/test_gpu_fft_table_half.py: which rows have half instances is read from the source, and every one of them
gets the case of its float32 twin."""
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


# ---- the float16 / bfloat16 instances (fft_half_kernels), the plan of tests/test_gpu_fft_table_half.py -----------------------
def _taps_of(L, M, q):
    from soxr_amd import device as dev
    return dev.Plan(*tp.rates_of(L, M), q).taps


def _hold_the_half_table(rows, macros, half):
    """Which rows have which half instances — from the source, against the float32 pointers of the same rows."""
    assert half["macros"]["HIPSOXR_HALF_ROW"] == list(tp.HALF_INSTANCES)
    assert half["macros"]["HIPSOXR_HALF_ROW_F32"] == list(tp.HALF_INSTANCES[:2]) + [None, None]
    keys = [(e["NA"], e["NB"], e["nt"]) for e in half["entries"]]
    assert len(set(keys)) == len(keys)          # (fft_half_kernels returns the first match: there is one)
    for r in rows:
        have, got = tp.instances_of(r, macros), tp.half_instances_of(r, half)
        want = [i for i in tp.HALF_INSTANCES if tp.FLOAT_TWIN[i] in have]
        assert got == want, (tp.row_name(r), got, want)
    # ... and the half table holds nothing the schedule table does not use
    used = {(r["M"] * r["k"], r["L"] * r["k"], half["nt_one_round"] if r["nt"] is None else r["nt"]) for r in rows}
    assert set(keys) == used, set(keys) ^ used


def test_the_half_table_follows_the_float32_pointers(table):
    """Every row with a pair2.f32 pointer has both half pair2 instances, every row with a strided2_cp.f32 pointer both half
    channel-pair instances, and no other row has any: 46 x 2 + 42 x 2 = 176 kernel instances."""
    rows, macros = table
    half = tp.parse_half()
    _hold_the_half_table(rows, macros, half)
    assert half["nt_one_round"] == 320
    n = {i: sum(i in tp.half_instances_of(r, half) for r in rows) for i in tp.HALF_INSTANCES}
    assert n == {("pair2", "f16"): 46, ("pair2", "bf16"): 46, ("strided2_cp", "f16"): 42, ("strided2_cp", "bf16"): 42}


def test_a_changed_half_table_is_noticed(table):
    """A HIPSOXR_HALF_ROW pointer turned into nullptr, two pointers swapped, a row dropped from an instantiation list, a row
    that matches by another thread count: none of these source texts passes."""
    rows, macros = table
    with open(tp.FFT_SRC) as f:
        text = f.read()
    _hold_the_half_table(rows, macros, tp.parse_half(text))
    ptr = "k_fft_strided2<PairOf<NA, NB, NT>, float, true, __bf16>},"
    spec = "X(4410, 1600, 320) "
    head = "#define HIPSOXR_HALF_ROW(NA, NB, NT) \\\n    {NA, NB, NT, "
    f16, bf16 = "k_fft_pair2<PairOf<NA, NB, NT>, float, _Float16>", "k_fft_pair2<PairOf<NA, NB, NT>, float, __bf16>"
    row = head + f16 + ", " + bf16 + ", \\\n"
    assert text.count(ptr) == 1 and text.count(spec) == 1 and text.count(row) == 1
    doctored = [text.replace(ptr, "nullptr},"),
                text.replace(spec, ""),
                text.replace(spec, "X(4410, 1600, 384) "),
                text.replace(row, head + bf16 + ", " + f16 + ", \\\n")]
    for t in doctored:
        assert t != text
        with pytest.raises(AssertionError):
            _hold_the_half_table(rows, macros, tp.parse_half(t))
    # (the float32 side: a row that loses its channel-pair pointer must lose the half ones with it)
    _, macros_cut = tp.parse_table(text.replace("k_fft_strided2<PairOf<NA, NB, NT>, float, true>, k_fft_strided2<PairOf<NA, NB, NT>, double, true>, \\",
                                                "nullptr, k_fft_strided2<PairOf<NA, NB, NT>, double, true>, \\"))
    assert macros_cut["HIPSOXR_PAIR"] != macros["HIPSOXR_PAIR"]
    with pytest.raises(AssertionError):
        _hold_the_half_table(rows, macros_cut, tp.parse_half(text))


def test_every_half_instance_has_the_case_of_its_float32_twin(table, plan):
    """A half job takes the row the float32 job of its shape takes: every half (row, instance, recipe) is a case or
    inadmissible exactly where the float32 instance of the same form is, under the same child, and none is unreachable."""
    rows, macros = table
    cases, status = plan
    half = tp.parse_half()
    hcases, hstatus = tp.case_plan(rows, macros, _taps_of, half=half)
    assert set(tp.children(rows)) == {"large", "small", "tiny", "k14", "k20"}
    assert {c["child"] for c in hcases} <= set(tp.children(rows))
    assert {k for k in hstatus} == {(tp.row_key(r), i, q) for r in rows for i in tp.half_instances_of(r, half) for q in tp.QUALITIES}
    child_of = {(c["row"], (c["form"], c["kind"]), c["quality"]): c for c in cases}
    for c in hcases:
        twin = child_of[(c["row"], tp.FLOAT_TWIN[(c["form"], c["kind"])], c["quality"])]
        assert (c["child"], c["hop"]) == (twin["child"], twin["hop"]), (c, twin)
    for (row, inst, q), st in hstatus.items():
        assert st in ("case", "inadmissible"), (row, inst, q, st)
        assert st == status[(row, tp.FLOAT_TWIN[inst], q)], (row, inst, q)
        assert inst[1] not in tp.WIDE_KINDS and (row, inst) not in tp.UNREACHABLE
    assert len({tp.case_id(c) for c in hcases}) == len(hcases)
    n_f32 = {form: sum((c["form"], c["kind"]) == (form, "f32") for c in cases) for form in ("pair2", "strided2_cp")}
    assert n_f32["pair2"] > 0 and n_f32["strided2_cp"] > 0
    for form in n_f32:
        for kind in ("f16", "bf16"):
            assert sum((c["form"], c["kind"]) == (form, kind) for c in hcases) == n_f32[form], (form, kind)
    assert len(hcases) == 2 * n_f32["pair2"] + 2 * n_f32["strided2_cp"]
    print(f"{len(hcases)} half cases: 2 x {n_f32['pair2']} unit-stride, 2 x {n_f32['strided2_cp']} channel-pair")


def test_the_half_bar_is_the_engines_plus_one_rounding():
    """half_bar: 4e-5 x RMS plus half the spacing of the type at |ref| + 4e-5 x RMS — at a binade edge the wider spacing,
    below the smallest normal the subnormal one."""
    import numpy as np
    ref = np.array([1.0, -1.0, 0.0, 3e-6])       # RMS 0.7071: s = 2.83e-5
    s = 4e-5 * tp.rms(ref)
    assert np.allclose(tp.half_bar(ref, "f16") - s, [2.0 ** -11, 2.0 ** -11, 2.0 ** -25, 2.0 ** -25], rtol=1e-6, atol=0)
    assert np.allclose(tp.half_bar(ref, "bf16") - s, [2.0 ** -8, 2.0 ** -8, 2.0 ** -24, 2.0 ** -23], rtol=1e-6, atol=0)
    assert tp.half_ulp(np.array([0.999]), "f16")[0] == 2.0 ** -12 and tp.half_ulp(np.array([1e-40]), "bf16")[0] == 2.0 ** -134


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
