#!/usr/bin/env python
"""Randomised differential check of the gradient family — the six adjoint selectors, both C entries (through
device.resample_tensor_adjoint and dist.resample_ragged_adjoint) and the two autograd pairs — against the float64 oracle.

    python tests/fuzz/fuzz_adjoint.py FAMILY [cases] [seed]          FAMILY: exact | interp | fast | ragged
    python tests/fuzz/fuzz_adjoint.py --draw FAMILY [cases] [seed]   print the drawn jobs as JSON and stop (no GPU, no library)

Honours HIPSOXR_LIBRARY (and HIPSOXR_DEBUG_LAUNCH_LOG on the debug-switch build: tests/test_gpu_adjoint_fuzz.py reads the launch
forms the draw reached from it).

DRAWING AND RUNNING ARE SEPARATE.  `draw(family, cases, seed)` returns plain dicts and imports neither torch nor the native
library (plan geometry comes from oracle/design.py, which tests/test_design_independent.py holds to the product's), so
tests/test_adjoint_fuzz_draw.py enumerates on the CPU exactly what a GPU run will do.  Attributes with a listed set of values
(size class, layout, type, selector, recipe) are dealt, not rolled: every value once while the case count allows, the rest by
weight, in shuffled order — a short run still meets every class.  No job exceeds 32768 frames per column or 2^20 elements.

FAMILIES, and what a case is compared with (every bound is one the fixed tests already use for the same arithmetic):
  exact   exact-bank plans under KERNEL_AUTO / _EXACT / _ADJOINT: the three give the same bits; tests/adjoint_ref.scatter on
          Plan.bank() per element — float64 1e-13 |A|^T|gy| + 1e-300, float32 (Tt + 2) 2^-24 |A32|^T|gy| on the bank rounded
          to float32 (tests/test_gpu_adjoint.py); float16 / bfloat16: the bits of the float32 job on gy.float() rounded once.
  interp  interpolated-phase plans under KERNEL_ADJOINT, half of the jobs at 8192 frames or more: 32 probe columns of the
          dense matrix (adjoint_ref.column: the oracle's forward on unit impulses, the engine's own coefficients) with the
          bounds of tests/test_gpu_adjoint_interp.py, and for the float64 job <A x, gy> = <x, gx> on three random x to 1e-12 of
          the probe columns' share of sum |x| |A|^T|gy| — the check that sees every position.  A float32 job against the float64
          job of the same cotangent, just pinned: 1e-6 relative RMS, 4e-5 x RMS pointwise.
  fast    KERNEL_ADJOINT_FFT / _TWO_STAGE / _AUTO against the float64 exact adjoint of the same cotangent on the GPU — which the
          same case holds to the oracle (scatter, or 16 probe columns and the identity).  Bars of tests/test_gpu_adjoint_fft.py
          and tests/test_gpu_adjoint_two_stage.py: 1e-6 relative RMS and 4e-5 x RMS pointwise (float32), 2e-9 VHQ / 1e-6 HQ
          (float64).  AUTO has the bits of the selector it resolves to.  A refusal ("unavailable") of KERNEL_ADJOINT_TWO_STAGE is
          predicted by the draw (tap count, 8192 frames either side); an unpredicted one fails, and at most one case in eight
          of a selector may end as a refusal.
  ragged  dist.resample_ragged_adjoint over 2 to 9 clips: each clip against the same clip run alone — the same bits under
          KERNEL_AUTO / _EXACT / _ADJOINT, the engine's class under KERNEL_ADJOINT_FFT, and under KERNEL_ADJOINT_AUTO on an
          interpolated-phase plan the class for the clips the two-stage form admits, the bits of KERNEL_ADJOINT for the rest —
          and four probe columns per clip against the oracle.
One case in six also goes through autograd: x.grad after backward(gy) has the bits of the adjoint called directly.

Output lines are written into out= views of NaN-filled buffers with 8 guard elements of 12345.0 either side of every column
(equal-length families).  A RuntimeError that is no refusal by name ("adjoint job:") ends the process at once with status 3:
nothing further is launched on the GPU."""
import json
import math
import os
import random
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for _p in (TESTS, os.path.join(ROOT, "python-soxr_amd"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import _adjoint_two_stage_probe as tp  # noqa: E402  (numpy only: poly_taps, smallest, MIN_FRAMES, F64_MAX_TAPS)

FAMILIES = ("exact", "interp", "fast", "ragged")
STD = [8000, 11025, 12000, 16000, 22050, 32000, 44100, 48000, 88200, 96000, 192000]  # fuzz_device_exact.py's
RECIPES = ["VHQ", "HQ", "MQ", "LQ", "QQ"]
QENUM = {"QQ": 0, "LQ": 1, "MQ": 2, "HQ": 4, "VHQ": 6}
PRIMES = [8209, 8219, 9973, 12289]  # above adjoint_rules.h kAdjMaxLc = 8192: a plan with one of them as L has no tile tables
# soxr_amd._native's values (run() asserts them): the draw does not import the library
AUTO, EXACT, ADJOINT, ADJOINT_FFT, ADJOINT_TWO_STAGE, ADJOINT_AUTO = 0, 6, 10, 11, 12, 13
SELECTOR_NAMES = {AUTO: "AUTO", EXACT: "EXACT", ADJOINT: "ADJOINT", ADJOINT_FFT: "ADJOINT_FFT", ADJOINT_TWO_STAGE: "ADJOINT_TWO_STAGE",
                  ADJOINT_AUTO: "ADJOINT_AUTO"}
INTERP_TILE = 256                        # _native.ADJOINT_INTERP_TILE (asserted)
MAX_FRAMES, MAX_ELEMS = 32768, 1 << 20
MAX_TAPS_F32 = 48                        # k_poly_adj: 56 taps have no table (tests/_adjoint_two_stage_probe.py UNREACHABLE)
# STD pairs KERNEL_ADJOINT_FFT answers "unavailable" for (measured, profiles/NOTES_adjoint_fuzz.md; and every 1:1 pair): left
# out of that selector's pool — the refusal cap stays where it is
FFT_NOT_SERVED = [{11025, 32000}, {12000, 32000}]
FFT_AUTO_MIN = 8192                     # job_rules.h kJobAutoFftMin: cotangent elements in all
LAYOUTS = ["interleaved", "planar", "clipstride", "chanslice"]
EXACT_N_X = ["1", "2", "T/2", "4Mc-1", "4Mc", "4Mc+1", "random", "64Mc+1"]
# (2 channels: the channel group by shift; 3: by division)
RAGGED_LANE_PLANS = [dict(plan=(44100, 48000, "HQ"), kind="f64", channels=2, lanes=32), dict(plan=(11025, 48000, "LQ"), kind=None, channels=3, lanes=16)]
RAGGED_LEN = ["0", "1", "short", "below4Mc", "from4Mc", "below8192", "from8192", "long"]
GUARD, POISON = 8, 12345.0
REL32, POINT = 1e-6, 4e-5                # tests/test_gpu_adjoint_fft.py, tests/test_gpu_adjoint_two_stage.py
REL64 = {"VHQ": 2e-9, "HQ": 1e-6}
REFUSAL_CAP = 8                          # at most one case in this many, per selector
FULL_PRODUCTS = 1 << 24                  # n_y T columns up to here: every column against scatter, above: three random ones


# =====================================================================================================================
# drawing (no torch, no native library)
# =====================================================================================================================
class Geo:
    """A plan's numbers from oracle/design.py, with the attribute names of device.Plan that the helpers read."""

    def __init__(self, in_rate, out_rate, quality):
        from oracle import design
        g = design.geometry(float(in_rate), float(out_rate), QENUM[quality])
        self.in_rate, self.out_rate, self.quality = float(in_rate), float(out_rate), quality
        self.L, self.M, self.taps, self.phases, self.att_db = int(g["L"]), int(g["M"]), int(g["T"]), int(g["phases"]), float(g["att_db"])

    def out_len(self, n):
        return (2 * int(n) * self.L + self.M) // (2 * self.M)

    @property
    def mc(self):  # adjoint_rules.h adj_tables: the replicated period, in input frames
        return max(-(-16 // self.M), -(-64 // self.L)) * self.M

    @property
    def terms(self):
        return math.ceil(self.taps * self.L / self.M) + 1

    def n_x_for(self, n_y):
        """the least n_x whose output holds n_y cotangent frames"""
        n = max(0, int(n_y * self.M / self.L) - 2)
        while self.out_len(n) < n_y:
            n += 1
        return n


def _spread(r, weighted, n):
    """n picks from [(item, weight)]: every item once while n allows, the rest by weight; shuffled"""
    items, weights = [it for it, _ in weighted], [w for _, w in weighted]
    out = items[:n]
    out += r.choices(items, weights, k=n - len(out))
    r.shuffle(out)
    return out


def _rates(i, o):
    return [i if isinstance(i, int) else float(i), o if isinstance(o, int) else float(o)]


def _ratio_ok(i, o, most):
    return max(i / o, o / i) <= most


def _cap_frames(geo, n_x, cols):
    """the largest n <= n_x with n and out_len(n) within the per-column and the per-job limits"""
    lim = min(MAX_FRAMES, MAX_ELEMS // cols)
    n = min(n_x, lim, max(1, lim * geo.M // geo.L + 1))
    while n > 1 and geo.out_len(n) > lim:
        n -= 1
    return n


def _shape(r, layout, channels, max_clips=4):
    """(rank, clips, channels) a layout can show itself on: a clip stride needs the clip axis, planar storage a channel axis"""
    rank = r.choice({"interleaved": [1, 2, 3], "planar": [2, 3], "clipstride": [3], "chanslice": [1, 2, 3]}[layout])
    if rank == 1:
        return 1, 1, 1
    return rank, (r.randint(1, max_clips) if rank == 3 else 1), channels


def _two_stage_predicted(geo, kind, n_x, n_y):
    """None where KERNEL_ADJOINT_TWO_STAGE serves the job, else why it answers "unavailable" (poly_design's tap count, the
    float64 table's LDS, two_stage_admits' frame counts)"""
    if not geo.phases or geo.quality not in ("HQ", "VHQ"):
        return "no form"
    try:
        taps = tp.poly_taps(geo)
    except StopIteration:
        return "taps"
    if taps > MAX_TAPS_F32 or (kind == "f64" and taps > tp.F64_MAX_TAPS):
        return "taps"
    return None if min(n_x, n_y) >= tp.MIN_FRAMES else "frames"


def _exact_plan(r, source, recipe, keep_recipe=False, fft_pool=False):
    """(in_rate, out_rate, recipe, Geo) of an exact-bank plan, ratio at most 6 either way.  fft_pool: the pool of
    KERNEL_ADJOINT_FFT by name, without the pairs that selector does not serve"""
    while True:
        if source == "std":
            i, o = r.choice(STD), r.choice(STD)
        elif source == "int":
            i, o = r.randint(1, 400), r.randint(1, 400)
        else:  # a prime above 8192 on one side
            p = r.choice(PRIMES)
            other = r.randint(p // 5, 5 * p)
            i, o = (other, p) if r.random() < 0.75 else (p, other)
        if not _ratio_ok(i, o, 6) or (fft_pool and (i == o or {i, o} in FFT_NOT_SERVED)):
            continue
        # (a long bank of a large L makes an interpolated-phase plan: a shorter recipe, or other rates)
        for q in [recipe] if keep_recipe else RECIPES[RECIPES.index(recipe):]:
            geo = Geo(i, o, q)
            if not geo.phases:
                return i, o, q, geo


def _interp_plan(r, kind_of_rate, recipe, most, cond=lambda geo: True):
    """(in_rate, out_rate, Geo) of an interpolated-phase plan"""
    tries = 0
    while True:
        tries += 1
        if kind_of_rate == "int" and (tries <= 200 or recipe in ("VHQ", "HQ", "MQ")):
            i, o = r.choice(STD), r.choice(STD) + r.choice([1, -1, 3, 11, -7])
            if r.random() < 0.5:
                i, o = o, i
        else:
            i = r.choice([r.uniform(8000, 96000), float(r.choice(STD))])
            o = r.choice([r.uniform(8000, 96000), r.choice(STD) + 0.25 * r.randint(1, 3)])
        if not _ratio_ok(i, o, most):
            continue
        geo = Geo(i, o, recipe)
        if geo.phases and cond(geo):
            return i, o, geo


def _common(family, idx, seed, i, o, q, geo):
    return dict(family=family, index=idx, seed=seed * 100003 + idx, rates=_rates(i, o), quality=q,
                L=geo.L, M=geo.M, taps=geo.taps, phases=geo.phases)


def _draw_exact(r, cases, seed):
    sources = _spread(r, [("std", 6), ("int", 3.5), ("prime", 0.5)], cases)
    recipes = _spread(r, [(q, 1) for q in RECIPES], cases)
    kinds = _spread(r, [("f32", 7), ("f64", 7), ("f16", 1), ("bf16", 1)], cases)
    classes = _spread(r, [(c, 1) for c in EXACT_N_X], cases)
    layouts = _spread(r, [(l, 1) for l in LAYOUTS], cases)
    channels = _spread(r, [(c, 1) for c in (1, 2, 3, 4, 5, 8, 70)], cases)
    cuts = _spread(r, [("full", 7), ("truncated", 4), ("empty", 1)], cases)
    grads = _spread(r, [(False, 5), (True, 1)], cases)
    out = []
    for idx in range(cases):
        i, o, q, geo = _exact_plan(r, sources[idx], recipes[idx])
        rank, clips, ch = _shape(r, layouts[idx], channels[idx])
        mc, cls = geo.mc, classes[idx]
        n_x = {"1": 1, "2": 2, "T/2": geo.taps // 2, "4Mc-1": 4 * mc - 1, "4Mc": 4 * mc, "4Mc+1": 4 * mc + 1,
               "random": r.randint(1, 6000), "64Mc+1": min(64 * mc + 1, 20000)}[cls]
        while clips > 1 and clips * ch * max(n_x, geo.out_len(n_x)) > MAX_ELEMS:
            clips -= 1
        capped = _cap_frames(geo, n_x, clips * ch)
        if capped != n_x:
            n_x, cls = capped, "capped"
        full = geo.out_len(n_x)
        n_y = {"full": full, "truncated": max(0, full - r.randint(0, 300)), "empty": 0}[cuts[idx]]
        c = _common("exact", idx, seed, i, o, q, geo)
        c.update(source=sources[idx], kind=kinds[idx], rank=rank, clips=clips, channels=ch, layout=layouts[idx], n_x=n_x, n_x_class=cls,
                 n_y=n_y, cut=cuts[idx], selectors=[AUTO, EXACT, ADJOINT], forward=EXACT,
                 autograd=bool(grads[idx]) and kinds[idx] in ("f32", "f64"), grad_selector=r.choice([AUTO, EXACT, ADJOINT]))
        out.append(c)
    return out


def _draw_interp(r, cases, seed):
    recipes = _spread(r, [(q, 1) for q in RECIPES], cases)
    # (integer pairs such as 48000 -> 44101 have interpolated phases from MQ up only: below, L T stays under the exact bank's limit)
    rate_kinds, n_long = [], 0
    for q in recipes:
        n_long += q in ("VHQ", "HQ", "MQ")
        rate_kinds.append("int" if q in ("VHQ", "HQ", "MQ") and n_long % 2 else "float")
    kinds = _spread(r, [("f32", 1), ("f64", 1)], cases)
    sizes = (["from8192", "below8192"] * cases)[:cases]  # half of the cases at 8192 frames or above
    r.shuffle(sizes)
    layouts = _spread(r, [(l, 1) for l in LAYOUTS], cases)
    channels = _spread(r, [(c, 1) for c in (1, 2, 3)], cases)
    cuts = _spread(r, [("full", 3), ("truncated", 1)], cases)
    grads = _spread(r, [(False, 5), (True, 1)], cases)
    out = []
    for idx in range(cases):
        big = sizes[idx] == "from8192"
        # (8192 frames in and at most 32768 out: at most 4:1 up for the long jobs)
        i, o, geo = _interp_plan(r, rate_kinds[idx], recipes[idx], 6, lambda g: not big or g.out_len(8192) <= MAX_FRAMES)
        rank, clips, ch = _shape(r, layouts[idx], channels[idx])
        if big:
            n_x = r.randint(8192, 20000)
        else:
            n_x = r.choice([1, 2, r.randint(3, 300), INTERP_TILE - 1, INTERP_TILE, INTERP_TILE + 1, r.randint(300, 8191), r.randint(300, 8191)])
        n_x = _cap_frames(geo, n_x, clips * ch)
        assert not big or n_x >= 8192
        full = geo.out_len(n_x)
        n_y = full if cuts[idx] == "full" else max(1, full - r.randint(0, 300))
        c = _common("interp", idx, seed, i, o, recipes[idx], geo)
        c.update(source=rate_kinds[idx], kind=kinds[idx], rank=rank, clips=clips, channels=ch, layout=layouts[idx], n_x=n_x,
                 n_x_class=sizes[idx], n_y=n_y, cut=cuts[idx] if n_y < full else "full", selectors=[ADJOINT], forward=EXACT,
                 autograd=bool(grads[idx]), grad_selector=ADJOINT)
        out.append(c)
    return out


def _draw_fast(r, cases, seed):
    n_auto = (cases + 1) // 2  # half of the cases AUTO, a quarter each named selector
    n_fft = (cases - n_auto + 1) // 2
    selectors = [ADJOINT_AUTO] * n_auto + [ADJOINT_FFT] * n_fft + [ADJOINT_TWO_STAGE] * (cases - n_auto - n_fft)
    r.shuffle(selectors)
    kinds = _spread(r, [("f32", 1), ("f64", 1)], cases)
    layouts = _spread(r, [(l, 1) for l in LAYOUTS], cases)
    channels = _spread(r, [(c, 1) for c in (1, 2, 3)], cases)
    n_sel = {s: selectors.count(s) for s in sorted(set(selectors))}
    auto_plans = (["exact-bank", "interp"] * cases)[:n_sel.get(ADJOINT_AUTO, 0)]
    r.shuffle(auto_plans)
    auto_exact_sizes = _spread(r, [("below", 1), ("at", 1), ("above", 1), ("random", 1)], auto_plans.count("exact-bank"))
    auto_exact_recipes = _spread(r, [(q, 1) for q in RECIPES], auto_plans.count("exact-bank"))
    interp_sizes = {ADJOINT_AUTO: _spread(r, [("smallest", 1), ("smallest-1", 1), ("smallest+1", 1), ("random", 1)], auto_plans.count("interp")),
                    ADJOINT_TWO_STAGE: _spread(r, [("smallest", 1), ("smallest+1", 1), ("random", 1), ("smallest-1", 1)], n_sel.get(ADJOINT_TWO_STAGE, 0))}
    refusals_left = n_sel.get(ADJOINT_TWO_STAGE, 0) // REFUSAL_CAP  # predicted refusals the cap leaves room for
    grads, owed = {s: _spread(r, [(True, 1), (False, 5)], n) for s, n in n_sel.items()}, {}
    out = []
    for idx in range(cases):
        sel, kind = selectors[idx], kinds[idx]
        rank, clips, ch = _shape(r, layouts[idx], channels[idx], max_clips=2)
        cols = clips * ch
        cut, predicted, resolves = "full", None, None
        if sel == ADJOINT_FFT or (sel == ADJOINT_AUTO and auto_plans.pop() == "exact-bank"):
            recipe = r.choice(["HQ", "VHQ"]) if sel == ADJOINT_FFT else auto_exact_recipes.pop()
            size = r.choice(["small", "mid", "long"]) if sel == ADJOINT_FFT else auto_exact_sizes.pop()
            while True:  # (the threshold jobs: the input of 8192 cotangent elements stays within the per-column limit)
                i, o, q, geo = _exact_plan(r, "std", recipe, keep_recipe=True, fft_pool=sel == ADJOINT_FFT)
                if size not in ("below", "at", "above") or geo.n_x_for(-(-FFT_AUTO_MIN // cols) + 1) <= MAX_FRAMES:
                    break
            if size in ("below", "at", "above"):  # the selector's threshold: 8192 cotangent elements in all
                n_y = {"below": (FFT_AUTO_MIN - 1) // cols, "at": -(-FFT_AUTO_MIN // cols), "above": -(-FFT_AUTO_MIN // cols) + 1}[size]
                n_x = geo.n_x_for(n_y)
                cut = "truncated" if n_y < geo.out_len(n_x) else "full"
            else:
                n_x = {"small": r.randint(64, 2000), "mid": r.randint(2000, 12000), "long": r.randint(12000, 20000), "random": r.randint(1, 20000)}[size]
                n_x = _cap_frames(geo, n_x, cols)
                n_y = geo.out_len(n_x)
                if r.random() < 0.25:
                    n_y, cut = max(1, n_y - r.randint(0, 300)), "truncated"
            if sel == ADJOINT_AUTO:
                resolves = ADJOINT_FFT if q in ("HQ", "VHQ") and n_y * cols >= FFT_AUTO_MIN else ADJOINT
        else:
            size = interp_sizes[sel].pop()
            want_refusal = sel == ADJOINT_TWO_STAGE and size == "smallest-1" and refusals_left > 0
            if sel == ADJOINT_TWO_STAGE and size == "smallest-1" and not want_refusal:
                size = "smallest"  # (the cap leaves no room: the admitted side of the threshold)
            recipe = r.choice(["HQ", "VHQ"])
            # a plan the form serves in this width (the fixed tests hold the others: tests/test_gpu_adjoint_auto.py)
            served = lambda g: _two_stage_predicted(g, kind, 1 << 20, 1 << 20) is None and g.out_len(tp.smallest(g) + 1) <= MAX_FRAMES
            i, o, geo = _interp_plan(r, r.choice(["int", "float"]), recipe, 3, served)
            q, n0 = recipe, tp.smallest(geo)
            hi = max(n0 + 1, _cap_frames(geo, MAX_FRAMES, cols))
            n_x = {"smallest": n0, "smallest-1": n0 - 1, "smallest+1": n0 + 1, "random": r.randint(n0, hi)}[size]
            n_y = geo.out_len(n_x)
            if size == "random" and n_y - 300 >= tp.MIN_FRAMES and r.random() < 0.25:
                n_y, cut = n_y - r.randint(0, 300), "truncated"
            predicted = _two_stage_predicted(geo, kind, n_x, n_y)
            if sel == ADJOINT_TWO_STAGE:
                assert (predicted is not None) == want_refusal, (predicted, size)
                refusals_left -= 1 if want_refusal else 0
            else:
                resolves, predicted = (ADJOINT_TWO_STAGE if predicted is None else ADJOINT), None
        # autograd is dealt per selector (one case in six, at least one each); a refused job hands its turn to the selector's next
        owed[sel] = owed.get(sel, 0) + bool(grads[sel].pop())
        grad = predicted is None and owed[sel] > 0
        owed[sel] -= grad
        c = _common("fast", idx, seed, i, o, q, geo)
        # (the forward runs on the exact engine: every frequency-domain launch in the launch log is then an adjoint's)
        c.update(kind=kind, rank=rank, clips=clips, channels=ch, layout=layouts[idx], n_x=n_x, n_x_class=size, n_y=n_y, cut=cut,
                 selectors=[sel], resolves=resolves, refusal=predicted, forward=EXACT, autograd=bool(grad), grad_selector=sel)
        out.append(c)
    return out


def _draw_ragged(r, cases, seed):
    groups = _spread(r, [("exact", 2), ("fft", 1), ("interp", 1), ("auto-interp", 1)], max(cases - 2, 0)) + ["exact"] * min(cases, 2)
    r.shuffle(groups)
    kinds = _spread(r, [("f32", 1), ("f64", 1)], cases)
    channels = _spread(r, [(c, 1) for c in (1, 2, 3)], cases)
    grads = _spread(r, [(False, 5), (True, 1)], cases)
    exact_selectors = _spread(r, [(AUTO, 1), (EXACT, 1), (ADJOINT, 1)], groups.count("exact"))
    lengths = _spread(r, [(c, 1) for c in RAGGED_LEN], 9 * cases)
    cuts = _spread(r, [("full", 6), ("truncated", 2), ("zero", 1)], 9 * cases)
    # k_adj_tile's narrower slabs, in ragged form: the first two exact-bank tables are 2 or 3 interleaved channels on plans whose
    # 64-lane slab is above the LDS limits (tests/test_gpu_adjoint_forms.py f_f64: Lc = 640 takes 16 lanes; Lc = 160 in float64: 32)
    steer = list(RAGGED_LANE_PLANS)
    out = []
    for idx in range(cases):
        group, kind, ch = groups[idx], kinds[idx], channels[idx]
        steered = None
        if group == "exact":
            sel = exact_selectors.pop()
            if steer:
                steered = steer.pop(0)
                (i, o, q), kind, ch = steered["plan"], steered["kind"] or kind, steered["channels"]
                geo = Geo(i, o, q)
                assert not geo.phases
            else:
                i, o, q, geo = _exact_plan(r, r.choice(["std", "std", "int"]), r.choice(RECIPES))
        elif group == "fft":
            i, o, q, geo = _exact_plan(r, "std", r.choice(["HQ", "VHQ"]), keep_recipe=True, fft_pool=True)
            sel = ADJOINT_FFT
        else:
            q = r.choice(["HQ", "VHQ"]) if group == "auto-interp" else r.choice(RECIPES)
            fits = lambda g: g.out_len(tp.smallest(g) + 1) <= MAX_FRAMES and (group != "auto-interp" or _two_stage_predicted(g, kind, 1 << 20, 1 << 20) is None)
            i, o, geo = _interp_plan(r, r.choice(["int", "float"]), q, 3 if group == "auto-interp" else 6, fits)
            sel = ADJOINT_AUTO if group == "auto-interp" else ADJOINT
        n_clips = r.randint(2, 9)
        edge = INTERP_TILE if geo.phases else 4 * geo.mc  # where the launch form (or the tile count) changes
        n0 = tp.smallest(geo) if group == "auto-interp" else geo.n_x_for(8192)
        rows, classes, budget = [], [], MAX_ELEMS // ch
        for c_idx in range(n_clips):
            cls, cut = lengths.pop(), cuts.pop()
            if c_idx == 0 and group == "auto-interp":
                cls, cut = "from8192", "full"   # every such table holds a clip the two-stage form admits
            if c_idx == 0 and steered:
                cls = "long"                    # ... and a steered table a clip the period-tiled kernel takes
            n_x = {"0": 0, "1": 1, "short": r.randint(2, 200), "below4Mc": edge - 1, "from4Mc": edge + r.randint(0, 1),
                   "below8192": n0 - 1, "from8192": n0 + r.randint(0, 1), "long": r.randint(9000, 14000)}[cls]
            if n_x:
                n_x = _cap_frames(geo, n_x, ch)
            full = geo.out_len(n_x)
            if max(n_x, full) > budget:  # (the job's 2^20 elements are spent: a short clip in its place)
                cls, n_x = "short", r.randint(2, 200)
                full = geo.out_len(n_x)
            budget -= max(n_x, full)
            n_y = {"full": full, "truncated": max(0, full - r.randint(0, 300)), "zero": 0}[cut]
            rows.append([n_x, n_y])
            classes.append(cls)
        admitted = [sel == ADJOINT_AUTO and _two_stage_predicted(geo, kind, n_x, n_y) is None for n_x, n_y in rows]
        c = _common("ragged", idx, seed, i, o, q, geo)
        c.update(group=group, kind=kind, channels=ch, lanes=steered["lanes"] if steered else None, mono_shape=bool(ch == 1 and r.random() < 0.5), rows=rows, row_classes=classes,
                 admitted=admitted, selectors=[sel], forward=EXACT, autograd=bool(grads[idx]), grad_selector=sel)
        out.append(c)
    return out


def draw(family, cases=24, seed=0):
    """The jobs of one run, as plain dicts (JSON-serialisable); deterministic in (family, cases, seed)."""
    assert family in FAMILIES, family
    r = random.Random("%s/%d/%d" % (family, cases, seed))
    return {"exact": _draw_exact, "interp": _draw_interp, "fast": _draw_fast, "ragged": _draw_ragged}[family](r, cases, seed)


def job_extent(case):
    """(the longest column's frames, elements in all: the larger side of every column) — what the size limits speak of"""
    if case["family"] == "ragged":
        per = [max(n_x, n_y) for n_x, n_y in case["rows"]]
        return max(per), sum(per) * case["channels"]
    full = (2 * case["n_x"] * case["L"] + case["M"]) // (2 * case["M"])  # (autograd cases also run the whole output length)
    n = max(case["n_x"], case["n_y"], full if case["autograd"] else 0)
    return n, n * case["clips"] * case["channels"]


# =====================================================================================================================
# running
# =====================================================================================================================
def _as3(t):
    return t[None, :, None] if t.ndim == 1 else (t[None] if t.ndim == 2 else t)


def _like_rank(t3, rank):
    return t3[0, :, 0] if rank == 1 else (t3[0] if rank == 2 else t3)


class CaseFailure(Exception):
    pass


class Refusal(Exception):
    pass


def _expect(cond, *what):
    if not cond:
        raise CaseFailure(" ".join(str(w) for w in what))


class Runner:
    def __init__(self, family, seed):
        import numpy as np
        import torch
        from oracle import oracle
        from soxr_amd import _native, device as dev, dist
        import _provider  # noqa: F401  (port mode on the product's bank)
        import adjoint_ref
        self.np, self.torch, self.oracle, self.dev, self.dist, self.ref = np, torch, oracle, dev, dist, adjoint_ref
        assert (AUTO, EXACT, ADJOINT, ADJOINT_FFT, ADJOINT_TWO_STAGE, ADJOINT_AUTO) == (
            _native.KERNEL_AUTO, _native.KERNEL_EXACT, _native.KERNEL_ADJOINT, _native.KERNEL_ADJOINT_FFT, _native.KERNEL_ADJOINT_TWO_STAGE,
            _native.KERNEL_ADJOINT_AUTO) and INTERP_TILE == _native.ADJOINT_INTERP_TILE
        self.family, self.plans, self.banks = family, {}, {}
        self.shares, self.refusals, self.ran = {}, {}, {}
        self.oracle_s = 0.0
        self.dtype = {"f32": torch.float32, "f64": torch.float64, "f16": torch.float16, "bf16": torch.bfloat16}

    # ---- plumbing ------------------------------------------------------------------------------------------------------
    def plan(self, case):
        key = (tuple(case["rates"]), case["quality"])
        if key not in self.plans:
            self.plans[key] = self.dev.Plan(case["rates"][0], case["rates"][1], case["quality"])
        p = self.plans[key]
        _expect((p.L, p.M, p.taps, p.phases) == (case["L"], case["M"], case["taps"], case["phases"]), "the draw's geometry is not the plan's",
                (p.L, p.M, p.taps, p.phases))
        return p

    def bank(self, case, f32=False):
        key = (tuple(case["rates"]), case["quality"], f32)
        if key not in self.banks:
            if len(self.banks) >= 4:
                self.banks.clear()
            b = self.plan(case).bank()
            self.banks[key] = b.astype(self.np.float32).astype(self.np.float64) if f32 and not case["phases"] else b
        return self.banks[key]

    def share(self, name, value):
        self.shares[name] = max(self.shares.get(name, 0.0), float(value))

    def gpu(self, fn, *a, **kw):
        """fn on the GPU.  A refusal by name becomes Refusal; any other RuntimeError — a HIP error, from torch or from the library —
        ends the process here: nothing further is launched."""
        try:
            out = fn(*a, **kw)
            self.torch.cuda.synchronize()
            return out
        except RuntimeError as e:
            if "adjoint job:" in str(e):
                raise Refusal(str(e))
            print("FATAL: a RuntimeError that is no refusal by name; no further GPU work:\n%s" % str(e)[:2000], flush=True)
            os._exit(3)

    def bits(self, t):
        t = t.contiguous()
        return t.view({2: self.torch.int16, 4: self.torch.int32, 8: self.torch.int64}[t.element_size()])

    def same_bits(self, a, b):
        return a.shape == b.shape and a.dtype == b.dtype and bool(self.torch.equal(self.bits(a), self.bits(b)))

    def rms(self, a):
        a = self.np.asarray(a, self.np.float64)
        return float(self.np.sqrt(self.np.mean(a * a))) if a.size else 0.0

    # ---- data and layouts ----------------------------------------------------------------------------------------------
    def cotangent(self, case, rng, n_y=None):
        """(host values [clips, n_y, ch] float64 — what the device tensor holds, exactly — and the device tensor in the case's
        layout and rank)"""
        np, torch = self.np, self.torch
        clips, ch, n_y, dt = case["clips"], case["channels"], case["n_y"] if n_y is None else n_y, self.dtype[case["kind"]]
        g = torch.from_numpy(rng.standard_normal((clips, n_y, ch)).astype(np.float32 if dt != torch.float64 else np.float64)).to(dt)
        host = g.double().numpy()
        g = g.cuda()
        layout = case["layout"]
        if layout == "planar":       # channel-first storage viewed channel-last
            t = g.permute(0, 2, 1).contiguous().permute(0, 2, 1)
        elif layout == "clipstride":  # every other clip of a larger batch
            big = torch.full((2 * clips, n_y, ch), 777.0, dtype=dt, device="cuda")
            big[::2] = g
            t = big[::2]
        elif layout == "chanslice":   # every other channel of a wider frame
            big = torch.full((clips, n_y, 2 * ch), 777.0, dtype=dt, device="cuda")
            big[..., ::2] = g
            t = big[..., ::2]
        else:
            t = g
        return host, _like_rank(t, case["rank"])

    def run_guarded(self, plan, case, gy, kernel, dtype=None):
        """one job through out= into a NaN-filled view, 8 guard elements of 12345.0 either side of every column (and, for the
        channel slice, the channels in between); -> the payload [clips, n_x, ch], a copy"""
        torch = self.torch
        clips, ch, n_x, dt = case["clips"], case["channels"], case["n_x"], dtype or gy.dtype
        layout = case["layout"]
        if layout == "planar":
            buf = torch.full((clips, ch, n_x + 2 * GUARD), POISON, dtype=dt, device="cuda")
            out3 = buf[:, :, GUARD:-GUARD].permute(0, 2, 1)
        elif layout == "chanslice":
            buf = torch.full((clips, n_x + 2 * GUARD, 2 * ch), POISON, dtype=dt, device="cuda")
            out3 = buf[:, GUARD:-GUARD, ::2]
        else:
            buf = torch.full((clips, n_x + 2 * GUARD, ch), POISON, dtype=dt, device="cuda")
            out3 = buf[:, GUARD:-GUARD]
        out3.fill_(float("nan"))
        out = _like_rank(out3, case["rank"])
        got = self.gpu(self.dev.resample_tensor_adjoint, plan, gy, n_x, out=out, kernel=kernel)
        _expect(got.data_ptr() == out.data_ptr() and got.shape == out.shape, "out= was not used")
        payload = out3.clone()
        _expect(bool(torch.isfinite(payload).all()), "a payload element was not written (selector %d)" % kernel)
        out3.fill_(POISON)
        _expect(bool((buf == POISON).all()), "a guard element was written (selector %d)" % kernel)
        return payload

    def columns(self, t3):
        """[clips, frames, ch] -> float64 [frames, clips * ch] on the host"""
        a = t3.double().cpu().numpy() if hasattr(t3, "cpu") else t3
        return a.transpose(1, 0, 2).reshape(a.shape[1], a.shape[0] * a.shape[2])  # (n_y may be 0)

    # ---- references ------------------------------------------------------------------------------------------------------
    def check_scatter(self, case, G, GX, f32, rng, name):
        """exact-bank plan: GX [n_x, C] against adjoint_ref.scatter of G [n_y, C], per element"""
        np = self.np
        n_y, C = G.shape
        n_x = GX.shape[0]
        if n_y == 0:
            _expect(not GX.any(), "no cotangent, but the gradient is not zero")
            return
        pick = np.arange(C) if n_y * case["taps"] * C <= FULL_PRODUCTS else np.sort(rng.choice(C, size=min(3, C), replace=False))
        t0 = time.time()
        want, mag = self.ref.scatter(case["L"], case["M"], self.bank(case, f32), G[:, pick], n_x)
        self.oracle_s += time.time() - t0
        terms = math.ceil(case["taps"] * case["L"] / case["M"]) + 1
        bound = (terms + 2) * 2.0 ** -24 * mag if f32 else 1e-13 * mag + 1e-300
        err = np.abs(GX[:, pick] - want)
        self.share(name, (err / np.maximum(bound, 1e-300)).max())
        bad = np.argwhere(err > bound)
        _expect(not len(bad), "%s: %d elements above the bound, the first at frame %d of column %d: error/bound %.4g"
                % (name, len(bad), bad[0][0] if len(bad) else -1, pick[bad[0][1]] if len(bad) else -1,
                   float((err / np.maximum(bound, 1e-300)).max())))

    def probe_columns(self, case, n_x, seams, rng, count, mode, f32_bank=False):
        """{frame a: column a of A [out_len(n_x)]} at adjoint_ref.probes' positions"""
        from types import SimpleNamespace
        pl = SimpleNamespace(L=case["L"], M=case["M"], T=case["taps"], phases=case["phases"])
        bank = self.bank(case, f32_bank)
        t0 = time.time()
        cols = {a: self.ref.column(self.oracle, pl, bank, a, n_x, mode) for a in self.ref.probes(n_x, seams, rng, count)}
        self.oracle_s += time.time() - t0
        return cols

    def check_probes(self, case, cols, G, GX, f32, name):
        """GX [n_x, C] at the probed frames against column . G, with the per-element bounds; -> {a: |A[:, a]| . |G|  [C]}"""
        np = self.np
        terms = math.ceil(case["taps"] * case["L"] / case["M"]) + 1
        mags = {}
        for a, col in cols.items():
            col = col[:G.shape[0]]
            _expect(np.count_nonzero(col) <= terms, "a column of A with more terms than ceil(T L / M) + 1")
            want, mag = col @ G, np.abs(col) @ np.abs(G)
            bound = (terms + 2) * 2.0 ** -24 * mag if f32 else 1e-13 * mag + 1e-300
            err = np.abs(GX[a] - want)
            self.share(name, (err / np.maximum(bound, 1e-300)).max() if err.size else 0.0)
            _expect((err <= bound).all(), "%s: frame %d: error/bound %.4g" % (name, a, float((err / np.maximum(bound, 1e-300)).max())))
            mags[a] = mag
        return mags

    def check_identity(self, case, mags, G, GX64, rng, name):
        """<A x, gy> = <x, gx> on three random x (A x: the oracle, port_f64), each on a random column, to 1e-12 of the probe
        columns' share of sum |x| |A|^T|gy| — a subset of the non-negative terms, so a tighter bound than the whole job's"""
        from types import SimpleNamespace
        np = self.np
        pl = SimpleNamespace(L=case["L"], M=case["M"], T=case["taps"], phases=case["phases"])
        n_x, n_y = GX64.shape[0], G.shape[0]
        n_out = int(self.oracle.lib().oracle_out_len(n_x, pl.L, pl.M))
        for _ in range(3):
            x, c = rng.standard_normal(n_x), int(rng.integers(0, G.shape[1]))
            t0 = time.time()
            ax = self.oracle.resample_channel(pl, x, "port_f64", n_out=n_out, bank=self.bank(case))[:n_y]
            self.oracle_s += time.time() - t0
            lhs, rhs = math.fsum(ax * G[:, c]), math.fsum(x * GX64[:, c])
            scale = sum(abs(x[a]) * m[c] for a, m in mags.items())
            self.share(name, abs(lhs - rhs) / (1e-12 * scale) if scale else 0.0)
            _expect(abs(lhs - rhs) <= 1e-12 * scale, "%s: |<A x, gy> - <x, gx>| = %.3g above 1e-12 x %.3g (column %d)" % (name, abs(lhs - rhs), scale, c))

    def check_bars(self, got, ref, rel_bar, point_bar, name):
        """the project's relative-RMS and pointwise bars over a result against its float64 reference (numpy, same shape)"""
        np = self.np
        err = np.asarray(got, np.float64) - ref
        scale = self.rms(ref)
        if scale == 0.0:
            _expect(not err.any(), "%s: the reference is zero, the result is not" % name)
            return
        rel, worst = self.rms(err) / scale, float(np.abs(err).max()) / scale
        self.share(name + " rel rms", rel / rel_bar)
        _expect(rel <= rel_bar, "%s: relative RMS %.3g above %.3g" % (name, rel, rel_bar))
        if point_bar is not None:
            self.share(name + " pointwise", worst / point_bar)
            _expect(worst <= point_bar, "%s: worst / RMS %.3g above %.3g" % (name, worst, point_bar))

    def hold_reference(self, case, G, REF, rng, probes):
        """the float64 exact adjoint REF [n_x, C] of G [n_y, C], held to the oracle"""
        if not case["phases"]:
            self.check_scatter(case, G, REF, False, rng, "float64 reference vs scatter")
            return
        cols = self.probe_columns(case, REF.shape[0], range(INTERP_TILE, REF.shape[0], INTERP_TILE), rng, probes, "port_f64")
        mags = self.check_probes(case, cols, G, REF, False, "float64 probes")
        self.check_identity(case, mags, G, REF, rng, "float64 identity")

    def autograd(self, plan, case, rng):
        """x.grad after backward(gy) has the bits of the adjoint called directly with the same selector"""
        torch, dev = self.torch, self.dev
        sel, dt = case["grad_selector"], self.dtype[case["kind"]]
        x3 = torch.from_numpy(rng.standard_normal((case["clips"], case["n_x"], case["channels"]))).to(dt).cuda()
        x = _like_rank(x3, case["rank"]).clone().requires_grad_()
        y = self.gpu(dev.resample_tensor, plan, x, kernel=case["forward"], grad_kernel=sel)
        _expect(y.grad_fn is not None, "no grad_fn")
        gy = torch.from_numpy(rng.standard_normal(tuple(y.shape))).to(dt).cuda()
        self.gpu(y.backward, gy)
        want = self.gpu(dev.resample_tensor_adjoint, plan, gy, case["n_x"], kernel=sel)
        _expect(x.grad is not None and self.same_bits(x.grad, want), "autograd: x.grad differs from the adjoint called directly (selector %d)" % sel)

    # ---- families --------------------------------------------------------------------------------------------------------
    def run_exact(self, case, rng):
        torch = self.torch
        plan = self.plan(case)
        host, gy = self.cotangent(case, rng)
        half = case["kind"] in ("f16", "bf16")
        res = {sel: self.run_guarded(plan, case, gy, sel) for sel in case["selectors"]}
        first = case["selectors"][0]
        _expect(self.same_bits(self.run_guarded(plan, case, gy, first), res[first]), "two runs differ in bits")
        for sel in case["selectors"][1:]:
            _expect(self.same_bits(res[sel], res[first]), "selector %d differs in bits from selector %d" % (sel, first))
        gx = res[first]
        if half:  # the float32 job on gy.float(), rounded once
            gx32 = self.run_guarded(plan, case, gy.float(), first, dtype=torch.float32)
            _expect(self.same_bits(gx, gx32.to(gx.dtype)), "the half job is not the float32 job rounded once")
            gx = gx32
        self.check_scatter(case, self.columns(host), self.columns(gx), case["kind"] != "f64", rng, "float32 vs scatter" if case["kind"] != "f64" else "float64 vs scatter")
        if case["n_y"] == 0:
            _expect(not bool(self.bits(gx).any()), "no cotangent: +0 everywhere")
        if case["autograd"]:
            self.autograd(plan, case, rng)

    def run_interp(self, case, rng):
        plan = self.plan(case)
        host, gy = self.cotangent(case, rng)
        got = self.run_guarded(plan, case, gy, ADJOINT)
        _expect(self.same_bits(self.run_guarded(plan, case, gy, ADJOINT), got), "two runs differ in bits")
        G, n_x = self.columns(host), case["n_x"]
        seams = range(INTERP_TILE, n_x, INTERP_TILE)
        if case["kind"] == "f64":
            gx64 = got
        else:
            gx64 = self.gpu(self.dev.resample_tensor_adjoint, plan, _as3(gy).double().contiguous(), n_x, kernel=ADJOINT)
        GX64 = self.columns(gx64)
        state = rng.bit_generator.state
        cols = self.probe_columns(case, n_x, seams, rng, 32, "port_f64")
        mags = self.check_probes(case, cols, G, GX64, False, "float64 probes")
        self.check_identity(case, mags, G, GX64, rng, "float64 identity")
        if case["kind"] == "f32":
            rng.bit_generator.state = state  # (the same positions)
            cols32 = self.probe_columns(case, n_x, seams, rng, 32, "port_f32")
            self.check_probes(case, cols32, G, self.columns(got), True, "float32 probes")
            self.check_bars(self.columns(got), GX64, REL32, POINT, "float32 vs float64 job")
        if case["autograd"]:
            self.autograd(plan, case, rng)

    def run_fast(self, case, rng):
        plan = self.plan(case)
        sel, kind, q, n_x = case["selectors"][0], case["kind"], case["quality"], case["n_x"]
        host, gy = self.cotangent(case, rng)
        G = self.columns(host)
        ref = self.gpu(self.dev.resample_tensor_adjoint, plan, _as3(gy).double().contiguous(), n_x, kernel=ADJOINT)
        REF = self.columns(ref)
        self.hold_reference(case, G, REF, rng, 16)
        self.ran[sel] = self.ran.get(sel, 0) + 1
        try:
            got = self.run_guarded(plan, case, gy, sel)
        except Refusal as e:
            _expect("unavailable" in str(e), "refused, but not as unavailable: %s" % e)
            _expect(case["refusal"] is not None or sel == ADJOINT_FFT, "a refusal the draw did not predict: %s" % e)
            self.refusals[sel] = self.refusals.get(sel, 0) + 1
            print("refusal, case %d: %s" % (case["index"], describe(case)))
            return
        _expect(case["refusal"] is None, "the draw predicted a refusal (%s), the job ran" % case["refusal"])
        _expect(self.same_bits(self.run_guarded(plan, case, gy, sel), got), "two runs differ in bits")
        named = sel
        if sel == ADJOINT_AUTO:
            named = case["resolves"]
            try:
                want = self.run_guarded(plan, case, gy, named)
            except Refusal as e:  # an engine that declines leaves the job to the exact adjoint
                _expect(named == ADJOINT_FFT and "unavailable" in str(e), "the selector AUTO should resolve to refuses: %s" % e)
                self.refusals["ADJOINT_FFT under AUTO"] = self.refusals.get("ADJOINT_FFT under AUTO", 0) + 1
                named = ADJOINT
                want = self.run_guarded(plan, case, gy, named)
            _expect(self.same_bits(got, want), "KERNEL_ADJOINT_AUTO differs in bits from selector %d" % named)
        GOT = self.columns(got)
        if named == ADJOINT:
            if kind == "f64":
                _expect(self.same_bits(got, ref), "the exact adjoint twice: different bits")
            else:
                self.check_bars(GOT, REF, REL32, POINT, "float32 exact adjoint vs float64")
        elif kind == "f32":
            self.check_bars(GOT, REF, REL32, POINT, "%s float32" % SELECTOR_NAMES[named])
        else:  # (float64: the pointwise bar is the two-stage form's)
            self.check_bars(GOT, REF, REL64[q], POINT if named == ADJOINT_TWO_STAGE else None, "%s float64 %s" % (SELECTOR_NAMES[named], q))
        if named == ADJOINT_TWO_STAGE:  # head and tail separately, per column
            scale = self.rms(REF)
            for part, tag in ((slice(0, 64), "head"), (slice(-64, None), "tail")):
                worst = float(self.np.abs(GOT[part] - REF[part]).max()) / scale
                self.share("ADJOINT_TWO_STAGE %s pointwise" % tag, worst / POINT)
                _expect(worst <= POINT, "two-stage %s: worst / RMS %.3g above %.3g" % (tag, worst, POINT))
        if case["autograd"]:
            self.autograd(plan, case, rng)

    def run_ragged(self, case, rng):
        np, torch, dev, dist = self.np, self.torch, self.dev, self.dist
        plan = self.plan(case)
        sel, kind, q, ch = case["selectors"][0], case["kind"], case["quality"], case["channels"]
        dt, f32 = self.dtype[kind], kind == "f32"
        shape = (lambda n: (n,)) if case["mono_shape"] else (lambda n: (n, ch))
        gys = [torch.from_numpy(rng.standard_normal(shape(n_y))).to(dt).cuda() for _, n_y in case["rows"]]
        n_xs = [n_x for n_x, _ in case["rows"]]
        self.ran[sel] = self.ran.get(sel, 0) + 1
        try:
            got = self.gpu(dist.resample_ragged_adjoint, plan, gys, n_xs, kernel=sel)
        except Refusal as e:
            _expect(sel == ADJOINT_FFT and "unavailable" in str(e), "refused: %s" % e)
            self.refusals[sel] = self.refusals.get(sel, 0) + 1
            print("refusal, case %d: %s" % (case["index"], describe(case)))
            return
        again = self.gpu(dist.resample_ragged_adjoint, plan, gys, n_xs, kernel=sel)
        bar = REL32 if f32 else REL64.get(q)
        if case["phases"]:
            seams, mode = (lambda n: range(INTERP_TILE, n, INTERP_TILE)), ("port_f32" if f32 else "port_f64")
        else:
            mc = max(-(-16 // case["M"]), -(-64 // case["L"])) * case["M"]
            seams, mode = (lambda n: sorted(set(range(64 * mc, n, 64 * mc)) | set(range((64 // ch) * mc, n, (64 // ch) * mc)))), "ref"
        for c, ((n_x, n_y), gy, gx) in enumerate(zip(case["rows"], gys, got)):
            tag = "clip %d (n_x %d, n_y %d)" % (c, n_x, n_y)
            _expect(tuple(gx.shape) == shape(n_x) and gx.dtype == dt, tag, "shape", tuple(gx.shape))
            _expect(self.same_bits(gx, again[c]), tag, "two runs differ in bits")
            if n_x == 0:
                continue
            _expect(bool(torch.isfinite(gx).all()), tag, "an element is not finite")
            fast = sel == ADJOINT_FFT or (sel == ADJOINT_AUTO and case["admitted"][c])
            alone = self.gpu(dev.resample_tensor_adjoint, plan, gy, n_x, kernel=ADJOINT if sel == ADJOINT_AUTO and not fast else sel)
            G, GX = gy.double().cpu().numpy().reshape(n_y, ch), gx.double().cpu().numpy().reshape(n_x, ch)
            if n_y == 0:
                _expect(not GX.any(), tag, "no cotangent, but the gradient is not zero")
                continue
            if not fast:
                _expect(self.same_bits(gx, alone), tag, "differs in bits from the clip run alone")
                held, held_f32, name = GX, f32, "ragged %s probes" % kind
            else:  # the engine's class against the clip alone; the values against the float64 exact adjoint, held to the oracle below
                ALONE = alone.double().cpu().numpy().reshape(n_x, ch)
                self.check_bars(GX, ALONE, bar, None, "ragged %s vs the clip alone" % SELECTOR_NAMES[sel])
                held = self.gpu(dev.resample_tensor_adjoint, plan, gy.double(), n_x, kernel=ADJOINT).cpu().numpy().reshape(n_x, ch)
                self.check_bars(GX, held, bar, POINT if f32 or sel == ADJOINT_AUTO else None, "ragged %s %s vs the float64 exact adjoint" % (SELECTOR_NAMES[sel], kind))
                held_f32, name = False, "ragged float64 reference probes"
            cols = self.probe_columns(case, n_x, seams(n_x), rng, 4, ("port_f32" if held_f32 else "port_f64") if case["phases"] else mode, f32_bank=held_f32)
            self.check_probes(case, cols, G, held, held_f32, name)
        if case["autograd"]:
            xs = [torch.from_numpy(rng.standard_normal(shape(n_x))).to(dt).cuda().requires_grad_() for n_x in n_xs]
            ys = self.gpu(dist.resample_ragged, plan, xs, kernel=case["forward"], grad_kernel=sel)
            gfull = [torch.from_numpy(rng.standard_normal(tuple(y.shape))).to(dt).cuda() for y in ys]
            grads = self.gpu(torch.autograd.grad, ys, xs, gfull)
            want = self.gpu(dist.resample_ragged_adjoint, plan, gfull, n_xs, kernel=sel)
            for c, (g, w) in enumerate(zip(grads, want)):
                _expect(self.same_bits(g, w), "autograd: clip %d's gradient differs from the ragged adjoint called directly" % c)


def describe(case):
    keys = ("rates", "quality", "kind", "rank", "clips", "channels", "layout", "n_x", "n_x_class", "n_y", "selectors", "resolves", "refusal", "rows", "group", "autograd")
    return " ".join("%s=%s" % (k, case[k]) for k in keys if k in case)


def run(family, cases=24, seed=0):
    import numpy as np
    jobs = draw(family, cases, seed)
    t_start = time.time()
    rn = Runner(family, seed)
    fails = 0
    t0 = time.time()
    for case in jobs:
        rng = np.random.default_rng(case["seed"])
        try:
            getattr(rn, "run_" + family)(case, rng)
        except CaseFailure as e:
            fails += 1
            print("FAIL case %d: %s\n     %s" % (case["index"], e, describe(case)), flush=True)
        except Refusal as e:
            fails += 1
            print("FAIL case %d: refused: %s\n     %s" % (case["index"], e, describe(case)), flush=True)
    elapsed = time.time() - t0
    for sel in sorted(set(rn.ran) | set(rn.refusals), key=str):
        n, ran = rn.refusals.get(sel, 0), rn.ran.get(sel, 0)
        print("adjoint fuzz %s: refusals %s: %d of %d cases" % (family, SELECTOR_NAMES.get(sel, sel), n, ran))
        if sel in rn.ran and n * REFUSAL_CAP > ran:
            fails += 1
            print("FAIL: more than one case in %d of selector %s ended as a refusal" % (REFUSAL_CAP, SELECTOR_NAMES[sel]))
    for name, v in sorted(rn.shares.items()):
        print("adjoint fuzz %s: largest share of the bound, %s: %.4g" % (family, name, v))
    print("adjoint fuzz %s: %d cases in %.1f s (CPU oracle %.1f s; %.1f s before the first case)" % (family, len(jobs), elapsed, rn.oracle_s, t0 - t_start))
    print("adjoint fuzz %s: %d failures in %d cases (seed %d)" % (family, fails, len(jobs), seed))
    return 1 if fails else 0


def main(argv):
    only_draw = argv[:1] == ["--draw"]
    if only_draw:
        argv = argv[1:]
    if not argv or argv[0] not in FAMILIES:
        print(__doc__.split("\n\n")[1], file=sys.stderr)
        return 2
    family, cases, seed = argv[0], int(argv[1]) if len(argv) > 1 else 24, int(argv[2]) if len(argv) > 2 else 0
    if only_draw:
        print(json.dumps(draw(family, cases, seed), indent=1))
        return 0
    return run(family, cases, seed)


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
