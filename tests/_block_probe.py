"""k_fft_block, the general path of the frequency-domain engine (csrc/fft.hip: one block per workgroup, run-time radix
schedule, real FFT through a half-length complex transform with untangle, multiply by H, tangle): its pass instances, read
from the source, a restatement of the geometry the host chooses for a job, and a job for every instance and layout.
Shared by tests/test_fft_block_plan.py (no GPU: the parse, the restatement, the case plan) and
tests/test_gpu_fft_block.py (the parent of the child processes).

PLAN PART (imports without a GPU).  An INSTANCE is (R, NB, SIGN) of `fft_pass<R, SIGN, NB>`: the `switch` of run_passes
names (R, NB) and the `per` threshold that chooses between two NB of a radix; k_fft_block calls run_passes<-1> (forward,
length A) and run_passes<+1> (inverse, length B).  geometry() restates factor_radices, fft_kept_run and the block search
of fft_geometry on L, M, T of oracle.plan; block_job() adds the instances a job of that geometry runs.  CASES is the plan:
off-table ratios the product serves on k_fft_block with no switch set (the small variant: fft_launch_block takes it below
2048 workgroups), each with the schedule it is expected to run, typed in — check_plan() holds that against the restatement
and the parsed instances, so an instance added, removed or re-thresholded in the source fails the host test until the plan
follows.  `python tests/_block_probe.py SEARCH` re-derives a cover from a grid of rates (and says whether an odd A or B
is reachable).

CHILD PART.  `python tests/_block_probe.py CHILD JOBS.npz RESULTS.npz` runs the jobs of an .npz file (written by the
test, which also holds their references) under the process's HIPSOXR_* environment — the debug-switch build with
HIPSOXR_DEBUG_LAUNCH_LOG, and HIPSOXR_FFT_LARGE_ONLY or HIPSOXR_FFT_NO_PAIR for two of the three children.  Per job: the
whole output buffer, guards and all (`y_<name>`), whether a second run gave the same bytes (`same_<name>`), and the launch
log's lines (`log_<name>`)."""
import json
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FFT_SRC = os.path.join(ROOT, "python-soxr_amd", "csrc", "fft.hip")
sys.path.insert(0, HERE)
import _table_probe as tp  # noqa: E402

NT = 256                    # threads of k_fft_block (__launch_bounds__(256, 2), dim3(256) in fft_launch_block)
MAX_HALF = 4096             # `Nin / 2 > 4096 || Nout / 2 > 4096` of fft_geometry
LARGE_MAX = 2600            # `std::max(Nin, Nout) / 2 > 2600`
LDS_BOUND = 150 * 1024      # `g.lds_bytes <= 150 * 1024`
AUTO_MIN = 1 << 13          # kJobAutoFftMin (job_rules.h)
AUTO, FFT = 0, 5            # hipsoxr_kernel_t
GUARD, POISON = 8, 12345.0
QUALITIES = ("HQ", "VHQ")
CHILDREN = {"plain": {}, "large": {"HIPSOXR_FFT_LARGE_ONLY": "1"}, "nopair": {"HIPSOXR_FFT_NO_PAIR": "1"}}


# ---------------------------------------------------------------------------------------------------------------------
# the instances, from the source
def run_passes_text(text=None):
    if text is None:
        with open(FFT_SRC) as f:
            text = f.read()
    m = re.search(r"template <int SIGN>\n__device__ __forceinline__ void run_passes\(.*?\n}\n", text, re.S)
    assert m, "run_passes was not found"
    return m.group(0)


def parse_run_passes(body=None, text=None):
    """-> dict rules: R -> [(per_max, NB), ..., (None, NB)] in the order the `case` tests them (None: otherwise);
    `default`: the radix of the default label; `signs`: the SIGN of every run_passes<...> call of k_fft_block."""
    if text is None:
        with open(FFT_SRC) as f:
            text = f.read()
    if body is None:
        body = run_passes_text(text)
    assert re.search(r"const int per = \(N / R \+ \(int\)blockDim\.x - 1\) / \(int\)blockDim\.x;", body), "the `per` rule changed"
    sw = body[body.index("switch (R)"):]
    sw = re.sub(r"//[^\n]*", "", sw[:sw.index("Ns *= R")])
    rules = {}
    inst = r"fft_pass<(\d+), SIGN, (\d+)>\(buf, N, Ns, W\);"
    labels = re.findall(r"\n\s*(case \d+|default):([^\n]*)", sw)
    assert labels, "no case of the switch was parsed"
    default = None
    for label, rest in labels:
        rest = rest.strip()
        m1 = re.fullmatch(inst + r" break;", rest)
        m2 = re.fullmatch(r"if \(per <= (\d+)\) " + inst + r" else " + inst + r" break;", rest)
        assert m1 or m2, "a case of run_passes has a form the parser does not know: " + rest
        if m1:
            R, lst = int(m1.group(1)), [(None, int(m1.group(2)))]
        else:
            assert m2.group(2) == m2.group(4), rest
            R, lst = int(m2.group(2)), [(int(m2.group(1)), int(m2.group(3))), (None, int(m2.group(5)))]
        if label == "default":
            default = R
        else:
            assert int(label.split()[1]) == R, rest
        assert R not in rules, R
        rules[R] = lst
    assert len(re.findall(r"fft_pass<", sw)) == sum(len(v) for v in rules.values()), "an fft_pass instance outside the parsed cases"
    signs = sorted(int(s) for s in re.findall(r"run_passes<([+-]1)>\(cur, [AB], a\.n[AB], a\.rad[AB], a\.W[AB]\);", text))
    return dict(rules=rules, default=default, signs=signs)


def tabs_lengths(text=None):
    """The transform lengths of HIPSOXR_SCHED_TABS_LIST: full lengths N_in / N_out whose passes have per-pass twiddle tables
    in the one-round kernels (pass_tables)."""
    if text is None:
        with open(FFT_SRC) as f:
            text = f.read()
    m = re.search(r"#define HIPSOXR_SCHED_TABS_LIST\(X\) \\\n([^\n]*)\n", text)
    assert m, "HIPSOXR_SCHED_TABS_LIST was not found"
    return sorted(int(n) for n in re.findall(r"X\((\d+),", m.group(1)))


def instances(parsed):
    """Every (R, NB, SIGN) the source instantiates."""
    return sorted((R, nb, s) for R, lst in parsed["rules"].items() for _, nb in lst for s in parsed["signs"])


def nb_of(parsed, N, R):
    """The NB run_passes takes for radix R of a length-N transform -> (R as dispatched, NB)."""
    per = (N // R + NT - 1) // NT
    if R not in parsed["rules"]:
        R = parsed["default"]          # (what the switch does; a radix the schedule holds and the switch lacks runs the default's pass)
    for per_max, nb in parsed["rules"][R]:
        if per_max is None or per <= per_max:
            return R, nb


# ---------------------------------------------------------------------------------------------------------------------
# the host's geometry (factor_radices, fft_kept_run, fft_geometry with force_k = 0), restated
def factor_radices(n):
    """-> the schedule, ascending, or None (not 7-smooth, or more than 8 passes)."""
    rad, twos = [], 0
    while n % 2 == 0:
        n //= 2
        twos += 1
    for pr in (7, 5, 3):
        while n % pr == 0:
            n //= pr
            rad.append(pr)
    if n != 1:
        return None
    rad += [16] * (twos // 4)
    if twos % 4:
        rad.append(1 << (twos % 4))
    rad.sort()
    return rad if 0 < len(rad) <= 8 else None


def kept_run(L, M, T, k):
    """-> (lead_periods, hop_periods); hop_periods < 1: no period is kept."""
    disc = ((T // 2 + 2) * L + M - 1) // M
    lead = (disc + L - 1) // L
    num = k * L - disc - lead * L
    return lead, (num // L if num >= 0 else -((-num) // L))      # (C++ division truncates; only `< 1` is asked of it)


def geometry(L, M, T, small):
    """fft_geometry(p, g, small, 0) -> dict k, A, B, radA, radB, lead_periods, hop_periods, v0, hop_out, lds_bytes, or None."""
    got = None
    k = 1
    while k <= 4096:
        Nin, Nout = M * k, L * k
        if Nin // 2 > MAX_HALF or Nout // 2 > MAX_HALF:
            break
        if not (Nin % 2 or Nout % 2 or Nin < 6 * T):
            ra, rb = factor_radices(Nin // 2), factor_radices(Nout // 2)
            if ra and rb:
                if got and (small or max(Nin, Nout) // 2 > LARGE_MAX):
                    break
                got = dict(k=k, A=Nin // 2, B=Nout // 2, radA=ra, radB=rb)
        k *= 2
    if not got:
        return None
    lead, hop = kept_run(L, M, T, got["k"])
    if hop < 1:
        return None
    got.update(lead_periods=lead, hop_periods=hop, v0=lead * L, hop_out=hop * L, lds_bytes=(max(got["A"], got["B"]) + 8) * 8)
    return got if got["lds_bytes"] <= LDS_BOUND else None


def block_geometry(L, M, T, variant):
    """What fft_launch_block takes: "large" = the default search (HIPSOXR_FFT_LARGE_ONLY, or >= 2048 workgroups); "small" =
    the small-block search where it is admissible and smaller (`gs.ok && gs.k < g.k`), else the default again."""
    g = geometry(L, M, T, False)
    if g and variant == "small":
        gs = geometry(L, M, T, True)
        if gs and gs["k"] < g["k"]:
            g = gs
    return g


def served(pl):
    """fft_job_eligible's share of the plan, and fft_geometry's QQ refusal: an exact-ratio plan of HQ / VHQ."""
    return pl.phases == 0 and pl.att_db >= 120.0


_table_ratios = None


def on_table(L, M):
    """The ratio has a row in the paired-kernel schedule table (fft_pairs): launch_fft_impl goes there first."""
    global _table_ratios
    if _table_ratios is None:
        _table_ratios = {(r["L"], r["M"]) for r in tp.parse_table()[0]}
    return (L, M) in _table_ratios


def sched(parsed, N, rad, sign):
    """The passes of one transform as run_passes dispatches them -> [(R, NB, SIGN)]."""
    return [nb_of(parsed, N, R) + (sign,) for R in rad]


def block_job(parsed, pl, variant):
    """pl: an oracle.Plan (or anything with L, M, T).  -> the geometry plus `fwd` / `inv` (the instance of every pass) and
    `instances` (their set), or None where k_fft_block does not serve the plan."""
    g = block_geometry(pl.L, pl.M, pl.T, variant)
    if not g:
        return None
    g["fwd"], g["inv"] = sched(parsed, g["A"], g["radA"], -1), sched(parsed, g["B"], g["radB"], +1)
    g["instances"] = set(g["fwd"]) | set(g["inv"])
    return g


def sched_text(passes):
    return " ".join("%d/%d" % p[:2] for p in passes)


def sched_of_text(text, sign):
    return [tuple(int(v) for v in t.split("/")) + (sign,) for t in text.split()]


# ---------------------------------------------------------------------------------------------------------------------
# The case plan: rates, quality, and what the job is expected to run — block periods, transform lengths, "R/NB" per pass
# — typed in from the search's report (`SEARCH`) and held against the restatement by check_plan.  Every case is the SMALL
# variant, what the product takes for a job of fewer than 2048 workgroups with no switch set, at a ratio outside the
# schedule table.  large: (k, A, B) of the large variant where it differs — run again in the child with
# HIPSOXR_FFT_LARGE_ONLY.  auto: the multi-block job is made long enough (>= 2^13 outputs) and sent with
# HIPSOXR_KERNEL_AUTO; everything else is asked for by name.  wide: also the planar batch, the channel slice and the
# impulse batch (one up-sampling, one down-sampling ratio, both with an odd v0).
# The rare instances have two transform lengths wherever two exist on the search's grid: (3,6) 4032 and 3528, (4,4) 4032
# and 2240, (5,4) 3200 and 4000, (8,2) 3200 and 3528; (7,3) runs at 4032 alone (3584 / 7 = 512 butterflies are two rounds).
CASES = [
    dict(rates=(11025, 32000), quality="VHQ", k=4, A=882, fwd="2/8 3/4 3/4 7/2 7/2", B=2560, inv="2/8 5/2 16/1 16/1", large=None, auto=True),
    dict(rates=(8000, 28000), quality="VHQ", k=1024, A=1024, fwd="4/2 16/1 16/1", B=3584, inv="2/8 7/2 16/1 16/1", large=None, auto=True, wide=True),
    dict(rates=(44100, 14000), quality="VHQ", k=128, A=4032, fwd="3/6 3/6 4/4 7/3 16/1", B=1280, inv="5/2 16/1 16/1", large=None, auto=True),
    dict(rates=(12000, 37800), quality="VHQ", k=128, A=1280, fwd="5/2 16/1 16/1", B=4032, inv="3/6 3/6 4/4 7/3 16/1", large=None),
    dict(rates=(40000, 11025), quality="VHQ", k=4, A=3200, fwd="5/4 5/4 8/2 16/1", B=882, inv="2/8 3/4 3/4 7/2 7/2", large=None, auto=True, wide=True),
    dict(rates=(8000, 25000), quality="VHQ", k=256, A=1024, fwd="4/2 16/1 16/1", B=3200, inv="5/4 5/4 8/2 16/1", large=None),
    dict(rates=(11025, 20000), quality="VHQ", k=4, A=882, fwd="2/8 3/4 3/4 7/2 7/2", B=1600, inv="4/2 5/2 5/2 16/1", large=None),
    dict(rates=(48000, 40000), quality="HQ", k=256, A=768, fwd="3/4 16/1 16/1", B=640, inv="5/2 8/1 16/1", large=(512, 1536, 1280), auto=True),
    dict(rates=(40000, 48000), quality="HQ", k=256, A=640, fwd="5/2 8/1 16/1", B=768, inv="3/4 16/1 16/1", large=(512, 1280, 1536)),
    dict(rates=(44100, 20000), quality="VHQ", k=16, A=3528, fwd="3/6 3/6 7/2 7/2 8/2", B=1600, inv="4/2 5/2 5/2 16/1", large=None, auto=True),
    dict(rates=(20000, 44100), quality="VHQ", k=16, A=1600, fwd="4/2 5/2 5/2 16/1", B=3528, inv="3/6 3/6 7/2 7/2 8/2", large=None),
    dict(rates=(35000, 16000), quality="VHQ", k=128, A=2240, fwd="4/4 5/2 7/2 16/1", B=1024, inv="4/2 16/1 16/1", large=None),
    dict(rates=(16000, 35000), quality="VHQ", k=128, A=1024, fwd="4/2 16/1 16/1", B=2240, inv="4/4 5/2 7/2 16/1", large=None, auto=True),
    dict(rates=(50000, 11025), quality="HQ", k=4, A=4000, fwd="2/8 5/4 5/4 5/4 16/1", B=882, inv="2/8 3/4 3/4 7/2 7/2", large=None),
    dict(rates=(11025, 50000), quality="HQ", k=4, A=882, fwd="2/8 3/4 3/4 7/2 7/2", B=4000, inv="2/8 5/4 5/4 5/4 16/1", large=None, auto=True),
    # N_in = 2240, like N_in = 3200 of 20000 -> 44100 above: a length with per-pass twiddle tables in the one-round kernels
    # (HIPSOXR_SCHED_TABS_LIST) beside an N_out without — fft_build once laid that table over WA and WB of such a geometry
    dict(rates=(35000, 32000), quality="HQ", k=64, A=1120, fwd="2/8 5/2 7/2 16/1", B=1024, inv="4/2 16/1 16/1", large=(128, 2240, 2048)),
]
# Ratios ON the table, served by k_fft_block under HIPSOXR_FFT_NO_PAIR alone (by name; the small variant, as above) and, the
# same jobs, by the paired kernels in the plain child: two implementations of one method.
NOPAIR_CASES = [
    dict(rates=(44100, 48000), quality="VHQ", k=16, A=1176, fwd="3/4 7/2 7/2 8/1", B=1280, inv="5/2 16/1 16/1"),
    dict(rates=(48000, 44100), quality="VHQ", k=16, A=1280, fwd="5/2 16/1 16/1", B=1176, inv="3/4 7/2 7/2 8/1"),
    dict(rates=(22050, 8000), quality="VHQ", k=16, A=3528, fwd="3/6 3/6 7/2 7/2 8/2", B=1280, inv="5/2 16/1 16/1"),
    dict(rates=(8000, 24000), quality="VHQ", k=2048, A=1024, fwd="4/2 16/1 16/1", B=3072, inv="3/4 4/4 16/1 16/1"),
]


def case_name(c):
    return "%d_%d_%s" % (c["rates"][0], c["rates"][1], c["quality"])


def typed_instances(c):
    return set(sched_of_text(c["fwd"], -1)) | set(sched_of_text(c["inv"], +1))


def check_plan(parsed, plan_of, cases=None, nopair=None):
    """Holds the plan to its conditions -> a list of what is wrong (empty: the plan stands).  plan_of(rates, quality) ->
    an oracle.Plan."""
    cases = CASES if cases is None else cases
    nopair = NOPAIR_CASES if nopair is None else nopair
    bad, covered = [], set()
    want = set(instances(parsed))
    for c, off_table in [(c, True) for c in cases] + [(c, False) for c in nopair]:
        name = case_name(c)
        pl = plan_of(c["rates"], c["quality"])
        if not served(pl):
            bad.append(f"{name}: not an HQ / VHQ exact-ratio plan")
            continue
        if on_table(pl.L, pl.M) == off_table:
            bad.append(f"{name}: the ratio {pl.L}/{pl.M} is {'on' if off_table else 'not on'} the schedule table")
        g = block_job(parsed, pl, "small")
        if not g:
            bad.append(f"{name}: k_fft_block has no geometry for the plan")
            continue
        got = (g["k"], g["A"], sched_text(g["fwd"]), g["B"], sched_text(g["inv"]))
        if got != (c["k"], c["A"], c["fwd"], c["B"], c["inv"]):
            bad.append(f"{name}: the plan says k A fwd B inv = {(c['k'], c['A'], c['fwd'], c['B'], c['inv'])}, the restatement {got}")
        if max(g["A"], g["B"]) > MAX_HALF or g["lds_bytes"] > LDS_BOUND:
            bad.append(f"{name}: A, B = {g['A']}, {g['B']} or {g['lds_bytes']} bytes of LDS are out of bounds")
        if not g["instances"] <= want:
            bad.append(f"{name}: runs {sorted(g['instances'] - want)}, which the source does not instantiate")
        if off_table:
            covered |= g["instances"] & typed_instances(c)
            gl = block_job(parsed, pl, "large")
            large = None if gl["k"] == g["k"] else (gl["k"], gl["A"], gl["B"])
            if large != c["large"]:
                bad.append(f"{name}: large variant {large}, the plan says {c['large']}")
    for i in sorted(want - covered):
        bad.append("instance fft_pass<%d, %+d, %d> is run by no product-reachable case" % (i[0], i[2], i[1]))
    for what, ok in (("an up-sampling case", any(c["A"] < c["B"] for c in cases)), ("a down-sampling case", any(c["A"] > c["B"] for c in cases)),
                     ("an HQ case", any(c["quality"] == "HQ" for c in cases)), ("a VHQ case", any(c["quality"] == "VHQ" for c in cases)),
                     ("a case whose large variant differs", any(c["large"] for c in cases)),
                     ("KERNEL_AUTO on half of the cases", 2 * sum(bool(c.get("auto")) for c in cases) >= len(cases)),
                     ("a wide up-sampling case", any(c.get("wide") and c["A"] < c["B"] for c in cases)),
                     ("a wide down-sampling case", any(c.get("wide") and c["A"] > c["B"] for c in cases)),
                     ("two cases whose N_in alone is a table length of the one-round kernels",
                      len({c["A"] for c in cases if 2 * c["A"] in tabs_lengths() and 2 * c["B"] not in tabs_lengths()}) >= 2)):
        if not ok:
            bad.append("the plan lacks " + what)
    return bad


# ---------------------------------------------------------------------------------------------------------------------
# jobs of a case: output lengths around the seams of its blocks, layouts, inputs
# layout -> (clips, channels of the view, channels of the tensor it is cut from, first channel of the view)
LAYOUTS = {"mono": (1, 1, 1, 0), "il3": (2, 3, 3, 0), "planar3": (3, 1, 1, 0), "slice": (2, 2, 5, 1), "imp16": (16, 1, 1, 0)}
BASE_LAYOUTS, WIDE_LAYOUTS = ("mono", "il3"), ("planar3", "slice")


def shortest_in(out_len, t, L, M):
    """The shortest input with at least t outputs."""
    n = max(1, t * M // L)
    while out_len(n) < t:
        n += 1
    while n > 1 and out_len(n - 1) >= t:
        n -= 1
    return n


def jobs_of(c, pl, g, child, index=0, twin=False):
    """The jobs of case c on geometry g (of `child`'s variant) -> dicts name, child, case, rates, quality, layout, tag, n_in,
    n_out, kernel, signal, and what the launch log must say (k, hop_out, lds, n_blocks; None for a twin: the paired kernels'
    business).  Lengths: `one` = exactly one block's kept run; `plus1` = one output more (up-sampling steps over some
    lengths: the first attainable one behind the seam); `multi` = two kept runs plus a seeded remainder — first, interior
    and partial last block — raised by whole runs to 2^13 outputs for a KERNEL_AUTO case, the input one frame longer
    where that makes its parity differ from the case's index (odd and even in_frames both occur)."""
    L, M, hop = pl.L, pl.M, g["hop_out"]
    auto = bool(c.get("auto")) and child == "plain" and not twin
    seed = [c["rates"][0], c["rates"][1], QUALITIES.index(c["quality"]), hop]
    r = int(np.random.default_rng(seed).integers(1, hop - 1))
    t = 2 * hop + r
    while auto and t < AUTO_MIN:
        t += hop
    n_multi = shortest_in(pl.out_len, t, L, M)
    if n_multi % 2 != index % 2 and pl.out_len(n_multi + 1) % hop:
        n_multi += 1
    lengths = [("one", shortest_in(pl.out_len, hop, L, M)), ("plus1", shortest_in(pl.out_len, hop + 1, L, M)), ("multi", n_multi)]
    jobs = []

    def add(tag, n_in, layout, kernel, signal="noise"):
        n_out = pl.out_len(n_in)
        name = "%s%s__%s__%s__%s" % ("twin__" if twin else "", case_name(c), child, tag, layout)
        log = None if twin else dict(k=g["k"], hop_out=hop, lds=g["lds_bytes"], n_blocks=(n_out + hop - 1) // hop)
        jobs.append(dict(name=name, child="plain" if twin else child, case=case_name(c), rates=list(c["rates"]), quality=c["quality"], layout=layout,
                         tag=tag, n_in=n_in, n_out=n_out, kernel=kernel, signal=signal, log=log, L=L, M=M))

    for tag, n_in in lengths:
        for layout in BASE_LAYOUTS + (WIDE_LAYOUTS if c.get("wide") and child == "plain" else ()):
            add(tag, n_in, layout, AUTO if auto and tag == "multi" else FFT)
    if c.get("wide") and child == "plain":
        add("multi", n_multi, "imp16", FFT, "impulses")       # (by name: an impulse batch need not be long)
    return jobs


def impulse_at(job_n_in, hop, L, M):
    """First of the 16 consecutive input positions of the impulse batch: the middle of the interior block's kept run."""
    return min(job_n_in - 16, (3 * hop // 2) * M // L)


def signal(job, hop):
    """The job's input columns [clips * channels, n_in] float32, clip-major: white noise at 0.25, or unit impulses."""
    clips, ch, _, _ = LAYOUTS[job["layout"]]
    n = job["n_in"]
    if job["signal"] == "impulses":
        x = np.zeros((clips * ch, n), np.float32)
        p0 = impulse_at(n, hop, job["L"], job["M"])
        for i in range(clips * ch):
            x[i, p0 + i] = 1.0
        return x
    # one master signal per (ratio, length): every layout of a job length shares its first columns, and their references
    rng = np.random.default_rng([job["rates"][0], job["rates"][1], n])
    return (rng.standard_normal((6, n)) * 0.25).astype(np.float32)[:clips * ch]


def payload(layout, n):
    """Index of the job's view inside its [clips, GUARD + n + GUARD, channels of the tensor] buffer."""
    _, ch, _, c0 = LAYOUTS[layout]
    return (slice(None), slice(GUARD, GUARD + n), slice(c0, c0 + ch))


def all_jobs(parsed, plan_of):
    """Every job of the three children -> (jobs, geometry per (case name, child))."""
    jobs, geoms = [], {}
    for i, c in enumerate(CASES):
        pl = plan_of(c["rates"], c["quality"])
        geoms[(case_name(c), "plain")] = g = block_job(parsed, pl, "small")
        jobs += jobs_of(c, pl, g, "plain", i)
        if c["large"]:
            geoms[(case_name(c), "large")] = gl = block_job(parsed, pl, "large")
            jobs += jobs_of(c, pl, gl, "large", i + 1)
    for i, c in enumerate(NOPAIR_CASES):
        pl = plan_of(c["rates"], c["quality"])
        geoms[(case_name(c), "nopair")] = g = block_job(parsed, pl, "small")
        jobs += jobs_of(c, pl, g, "nopair", i)
        jobs += jobs_of(c, pl, g, "nopair", i, twin=True)
    return jobs, geoms


# ---------------------------------------------------------------------------------------------------------------------
# SEARCH: a cover of the parsed instances from a grid of rates, re-derived
SEARCH_RATES = (8000, 11025, 12000, 14000, 16000, 20000, 22050, 24000, 25000, 28000, 32000, 35000, 36000, 37800, 40000, 42000, 44100,
                48000, 50000, 56000, 64000, 72000, 75000, 88200, 96000, 100000, 112000, 128000, 176400, 192000)


def search(parsed, rates=SEARCH_RATES):
    """-> (rows, odd): rows = (rates, quality, variant, geometry) of every off-table job k_fft_block serves on the grid;
    odd = those with an odd A or B.  (None can exist: k = 1 needs L and M both even, a block of k = 2 periods keeps none —
    hop_periods = k - 2 lead_periods — so k >= 4 and A = M k / 2, B = L k / 2 are even.  For the same reason hop_out is even.)"""
    from oracle import design

    class P:
        pass
    rows, odd = [], []
    for fi in rates:
        for fo in rates:
            if fi == fo:
                continue
            for q in QUALITIES:
                d = design.geometry(float(fi), float(fo), {"HQ": 4, "VHQ": 6}[q])
                p = P()
                p.L, p.M, p.T, p.phases, p.att_db = d["L"], d["M"], d["T"], d["phases"], d["att_db"]
                if not served(p) or on_table(p.L, p.M):
                    continue
                for variant in ("small", "large"):
                    g = block_job(parsed, p, variant)
                    if g:
                        rows.append(((fi, fo), q, variant, g))
                        if g["A"] % 2 or g["B"] % 2 or g["hop_out"] % 2:
                            odd.append(rows[-1])
    return rows, odd


def _search_main():
    sys.path.insert(0, ROOT)
    parsed = parse_run_passes()
    rows, odd = search(parsed)
    print("%d jobs served on the grid; an odd A, B or hop_out: %d" % (len(rows), len(odd)))
    for inst in instances(parsed):
        mine = [r for r in rows if r[2] == "small" and inst in r[3]["instances"]]
        lens = sorted({r[3]["A"] if inst[2] < 0 else r[3]["B"] for r in mine})
        print("fft_pass<%d, %+d, %d>: %d jobs, transform lengths %s" % (inst[0], inst[2], inst[1], len(mine), lens))
        for r in mine[:4]:
            g = r[3]
            print("    %d -> %d %s  k %d  A %d [%s]  B %d [%s]  v0 %d  hop_out %d" % (r[0] + (r[1], g["k"], g["A"], sched_text(g["fwd"]), g["B"],
                                                                                      sched_text(g["inv"]), g["v0"], g["hop_out"])))


# ---------------------------------------------------------------------------------------------------------------------
# the child process
def _child_main(jobs_path, results_path):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "python-soxr_amd"))
    import torch
    from soxr_amd import device as dev
    data = np.load(jobs_path)
    jobs = json.loads(str(data["meta"]))
    log = tp.LogTail(os.environ["HIPSOXR_DEBUG_LAUNCH_LOG"])
    plans, out = {}, {}
    for job in jobs:
        name = job["name"]
        key = (job["rates"][0], job["rates"][1], job["quality"])
        if key not in plans:
            plans[key] = dev.Plan(*key)
        plan = plans[key]
        clips, ch, ch_all, c0 = LAYOUTS[job["layout"]]
        n_in, n_out = job["n_in"], job["n_out"]
        assert plan.out_len(n_in) == n_out, (name, plan.out_len(n_in), n_out)
        cols = data["x_" + name].reshape(clips, ch, n_in)
        # the input: a view inside a NaN-filled tensor — guard frames either side, NaN in the channels beside a slice
        xb = np.full((clips, n_in + 2 * GUARD, ch_all), np.nan, np.float32)
        xb[payload(job["layout"], n_in)] = cols.transpose(0, 2, 1)
        xt = torch.from_numpy(xb).cuda()
        yb = np.full((clips, n_out + 2 * GUARD, ch_all), POISON, np.float32)
        yb[payload(job["layout"], n_out)] = np.nan
        fill = torch.from_numpy(yb).cuda()
        xv = xt[payload(job["layout"], n_in)]
        runs = []
        log.take()
        try:
            for _ in range(2):
                buf = fill.clone()
                yv = buf[payload(job["layout"], n_out)]
                if job["layout"] == "mono":
                    dev.resample_tensor(plan, xv[0, :, 0], out=yv[0, :, 0], kernel=job["kernel"])
                else:
                    dev.resample_tensor(plan, xv, out=yv, kernel=job["kernel"])
                torch.cuda.synchronize()
                runs.append(buf.cpu().numpy())
                if len(runs) == 1:
                    lines = log.take()
        except RuntimeError as e:          # a refusal or a device error: nothing more is started on the device
            out["err_" + name] = np.array(str(e))
            break
        out["y_" + name] = runs[0]
        out["same_" + name] = np.array(runs[0].tobytes() == runs[1].tobytes())
        out["log_" + name] = np.array(json.dumps(lines))
        print("BLOCK_JOB", name, flush=True)
    np.savez(results_path, **out)
    print("BLOCK_PROBE done: %d jobs" % sum(k.startswith("y_") for k in out))


if __name__ == "__main__":
    if sys.argv[1] == "SEARCH":
        _search_main()
    elif sys.argv[1] == "CHILD":
        _child_main(sys.argv[2], sys.argv[3])
    else:
        raise SystemExit("usage: _block_probe.py SEARCH | CHILD JOBS.npz RESULTS.npz")


