"""The paired-block schedule table of the frequency-domain engine (csrc/fft.hip, fft_pairs), read from the source, and a
job for every kernel instance in it.  Shared by tests/test_fft_table.py (no GPU: the parse, the case plan, the float64
overlap-save model alone), tests/test_gpu_fft_table.py (the parent of the child processes) and
tools/make_fft_table_floor.py (the fixture tests/golden/fft_table_floor.json).

Run as a program (`_table_probe.py <child name>`, the debug-switch build loaded through HIPSOXR_LIBRARY, the child's
switches and HIPSOXR_DEBUG_LAUNCH_LOG in the environment) it runs every case of that child on the GPU and prints one JSON
line, "TABLE_PROBE {...}": per case whether it held, what failed, and the largest figures measured.

A ROW is (L, M, k, small) of a HIPSOXR_PAIR / HIPSOXR_PAIR_F32 line; an INSTANCE is (form, kind), one kernel pointer of
PairEntry: form pair2 (unit-stride columns, two blocks per transform), strided2_cp (interleaved channel pairs, one block of
two channels per transform), strided2_st (strided columns, two blocks per transform); kind f32, f64, f32on64 (float32
samples on float64 arithmetic, HIPSOXR_KERNEL_FFT_F64), i16, i32 (HIPSOXR_KERNEL_FFT_PCM).

The float16 / bfloat16 forms of a row (fft_half_kernels: HIPSOXR_HALF_ROW / HIPSOXR_HALF_ROW_F32 over the instantiation
lists) are HALF_INSTANCES, kinds f16 and bf16: parsed by parse_half, planned by case_plan(..., half=...), run by
`_table_probe.py half:<child name>` for tests/test_gpu_fft_table_half.py — a module and children of their own."""
import json
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FFT_SRC = os.path.join(ROOT, "python-soxr_amd", "csrc", "fft.hip")
FLOOR_JSON = os.path.join(HERE, "golden", "fft_table_floor.json")

# PairEntry's kernel pointers, in the struct's order (fft_launch_paired picks a field by layout, element type and selector)
INSTANCES = (("pair2", "f32"), ("pair2", "f64"), ("pair2", "f32on64"), ("strided2_cp", "f32"), ("strided2_cp", "f64"),
             ("strided2_st", "f32"), ("strided2_st", "f64"), ("pair2", "i16"), ("pair2", "i32"), ("strided2_cp", "i16"))
# HalfKernels' kernel pointers, in the struct's order (fft_launch_paired: by layout and element type)
HALF_INSTANCES = (("pair2", "f16"), ("pair2", "bf16"), ("strided2_cp", "f16"), ("strided2_cp", "bf16"))
WIDE_KINDS = ("f64", "f32on64", "i32")          # float64 arithmetic (`f64` of FftJobView)
# float32 unit-stride columns and their half forms: the jobs of fft_one_round_pick (`j.elem == HIPSOXR_F32 || v.half`)
F32_UNIT = (("pair2", "f32"), ("pair2", "f16"), ("pair2", "bf16"))
FLOAT_TWIN = {("pair2", "f16"): ("pair2", "f32"), ("pair2", "bf16"): ("pair2", "f32"),
              ("strided2_cp", "f16"): ("strided2_cp", "f32"), ("strided2_cp", "bf16"): ("strided2_cp", "f32")}
QUALITIES = ("VHQ", "HQ")
FFT, FFT_F64, FFT_PCM = 5, 8, 9                 # hipsoxr_kernel_t


# ---------------------------------------------------------------------------------------------------------------------
# the table, from the source
def _macro_body(text, name):
    m = re.search(r"#define " + name + r"\([^)]*\)((?:[^\n]*\\\n)*[^\n]*)\n", text)
    assert m, name
    body = m.group(1).replace("\\\n", " ")
    return body[body.index("{") + 1:body.rindex("}")]


def _split_top(s):
    out, depth, cur = [], 0, ""
    for ch in s:
        if ch in "<(":
            depth += 1
        elif ch in ">)":
            depth -= 1
        if ch == "," and depth == 0:
            out.append(cur.strip())
            cur = ""
        else:
            cur += ch
    out.append(cur.strip())
    return out


def _instance_of(expr):
    """A PairEntry initialiser -> (form, kind), or None for nullptr."""
    if expr == "nullptr":
        return None
    m = re.fullmatch(r"k_fft_pair2<PairOf<[^>]*>, (float|double)(?:, (float|int16_t|int32_t))?>", expr)
    if m:
        kind = {("float", None): "f32", ("double", None): "f64", ("double", "float"): "f32on64",
                ("float", "int16_t"): "i16", ("double", "int32_t"): "i32"}[m.groups()]
        return ("pair2", kind)
    m = re.fullmatch(r"k_fft_strided2<PairOf<[^>]*>, (float|double), (true|false)(?:, (int16_t))?>", expr)
    assert m, expr
    real, cp, io = m.groups()
    return ("strided2_cp" if cp == "true" else "strided2_st", "i16" if io else {"float": "f32", "double": "f64"}[real])


def parse_table(text=None):
    """-> (rows, macros).  rows: dicts L, M, k, small, NA, NB, nt (None: FFT_ONE_ROUND_NT), macro; in the table's order.
    macros: name -> the (form, kind) or None of each of the ten pointers, as the #define writes them."""
    if text is None:
        with open(FFT_SRC) as f:
            text = f.read()
    macros = {}
    for name in ("HIPSOXR_PAIR", "HIPSOXR_PAIR_F32"):
        parts = _split_top(_macro_body(text, name))
        assert parts[:3] == ["L", "M", "k"], parts[:5]
        macros[name] = [_instance_of(e) for e in parts[5:]]
    m = re.search(r"static const PairEntry pairs\[\] = \{(.*?)\n    \};", text, re.S)
    assert m, "fft_pairs: the table was not found"
    body = re.sub(r"//[^\n]*", "", m.group(1))
    rows = []
    pat = re.compile(r"HIPSOXR_PAIR(_F32)?\(([^()]*)\)")
    for mm in pat.finditer(body):
        a = [s.strip() for s in mm.group(2).split(",")]
        if mm.group(1):
            assert len(a) == 5, a
            L, M, k, NA, NB = map(int, a)
            rows.append(dict(L=L, M=M, k=k, small=3, NA=NA, NB=NB, nt=None, macro="HIPSOXR_PAIR_F32"))
        else:
            assert len(a) == 7, a
            small = {"false": 0, "true": 1}.get(a[3])
            small = int(a[3]) if small is None else small
            L, M, k, NA, NB, nt = (int(a[i]) for i in (0, 1, 2, 4, 5, 6))
            rows.append(dict(L=L, M=M, k=k, small=small, NA=NA, NB=NB, nt=nt, macro="HIPSOXR_PAIR"))
    rest = pat.sub("", body)
    assert not rest.replace(",", "").strip(), "fft_pairs holds an entry that is not a HIPSOXR_PAIR* row: " + rest.strip()[:200]
    for r in rows:
        assert r["NA"] == r["M"] * r["k"] and r["NB"] == r["L"] * r["k"], r
    return rows, macros


def row_key(r):
    return (r["L"], r["M"], r["k"], r["small"])


def row_name(r):
    return "%d:%d:k%d:s%d" % row_key(r)


def instances_of(row, macros):
    return [i for i in macros[row["macro"]] if i is not None]


def _half_instance_of(expr):
    """A HalfKernels initialiser -> (form, kind), or None for nullptr."""
    if expr == "nullptr":
        return None
    kinds = {"_Float16": "f16", "__bf16": "bf16"}
    m = re.fullmatch(r"k_fft_pair2<PairOf<NA, NB, NT>, float, (_Float16|__bf16)>", expr)
    if m:
        return ("pair2", kinds[m.group(1)])
    m = re.fullmatch(r"k_fft_strided2<PairOf<NA, NB, NT>, float, true, (_Float16|__bf16)>", expr)
    assert m, expr
    return ("strided2_cp", kinds[m.group(1)])


def parse_half(text=None):
    """The float16 / bfloat16 table of fft_half_kernels -> dict macros: name -> the (form, kind) or None of the four
    pointers of HIPSOXR_HALF_ROW / HIPSOXR_HALF_ROW_F32, as the #define writes them; entries: dicts NA, NB, nt, macro, list —
    the HIPSOXR_PART*_SPECS lists that `halves[]` expands, in its order; nt_one_round: FFT_ONE_ROUND_NT."""
    if text is None:
        with open(FFT_SRC) as f:
            text = f.read()
    macros = {}
    for name in ("HIPSOXR_HALF_ROW", "HIPSOXR_HALF_ROW_F32"):
        parts = _split_top(_macro_body(text, name))
        assert parts[:3] == ["NA", "NB", "NT"] and len(parts) == 3 + len(HALF_INSTANCES), parts
        macros[name] = [_half_instance_of(e) for e in parts[3:]]
    nt_one_round = int(re.search(r"#define FFT_ONE_ROUND_NT (\d+)", text).group(1))
    m = re.search(r"static const HalfKernels halves\[\] = \{(.*?)\n    \};", text, re.S)
    assert m, "fft_half_kernels: the table was not found"
    body = re.sub(r"//[^\n]*", "", m.group(1))
    pat = re.compile(r"(HIPSOXR_PART\d+_SPECS)\((HIPSOXR_HALF_ROW(?:_F32)?)\)")
    assert not pat.sub("", body).strip(), "fft_half_kernels holds an entry that is not a list of specs: " + body.strip()[:200]
    entries = []
    for lst, macro in pat.findall(body):
        line = re.search(r"#define " + lst + r"\(X\)([^\n]*)\n", text)
        assert line, lst
        specs = re.findall(r"X\(([^()]*)\)", line.group(1))
        assert specs and not re.sub(r"X\([^()]*\)", "", line.group(1)).strip(), lst
        for s in specs:
            na, nb, nt = (t.strip() for t in s.split(","))
            entries.append(dict(NA=int(na), NB=int(nb), nt=nt_one_round if nt == "FFT_ONE_ROUND_NT" else int(nt), macro=macro, list=lst))
    return dict(macros=macros, entries=entries, nt_one_round=nt_one_round)


def half_instances_of(row, half):
    """The half instances fft_half_kernels finds for a row: the first entry with the row's (M k, L k, threads)."""
    nt = half["nt_one_round"] if row["nt"] is None else row["nt"]
    for e in half["entries"]:
        if (e["NA"], e["NB"], e["nt"]) == (row["M"] * row["k"], row["L"] * row["k"], nt):
            return [i for i in half["macros"][e["macro"]] if i is not None]
    return []


def rates_of(L, M):
    """A rate pair of the ratio out / in = L / M."""
    g = max(1, 48000 // max(L, M))
    return M * g, L * g


# ---------------------------------------------------------------------------------------------------------------------
# the arithmetic of fft_kept_run (csrc/fft.hip), restated
def lead_periods(L, M, T):
    disc = ((T // 2 + 2) * L + M - 1) // M
    return (disc + L - 1) // L


def hop_out(L, M, T, k):
    """fft_geometry(force_k = k) / fft_hop_out (both through fft_kept_run): outputs a block of k periods keeps; 0: the row is not admissible for T taps."""
    if M * k // 2 > 4096 or L * k // 2 > 4096:
        return 0
    disc = ((T // 2 + 2) * L + M - 1) // M
    num = L * k - disc - lead_periods(L, M, T) * L
    hop_periods = num // L if num >= 0 else -1
    if hop_periods < 1 or 2 * hop_periods * L < L * k:
        return 0
    return hop_periods * L


# one child process per switch setting; a float32-only row (HIPSOXR_PAIR_F32) of k periods gets the child "k<k>"
BASE_CHILDREN = {"large": {"HIPSOXR_FFT_LARGE_ONLY": "1"},
                 "small": {"HIPSOXR_FFT_SMALL_ONLY": "1", "HIPSOXR_FFT_NO_TINY": "1"},
                 "tiny": {"HIPSOXR_FFT_SMALL_ONLY": "1"}}


def children(rows):
    out = dict(BASE_CHILDREN)
    for r in rows:
        if r["small"] == 3:
            out["k%d" % r["k"]] = {"HIPSOXR_DEBUG_FFT_K": str(r["k"])}
    return out


def pick_row(ratio_rows, T, env, wide, f32_unit, macros):
    """The row fft_choose_row chooses for a job of a few work items (far below every size threshold) of this ratio, under
    the switches of `env`; None: no paired kernel.  wide: float64 arithmetic.  f32_unit: float32 unit-stride columns."""
    large, small_only, no_tiny = ("HIPSOXR_FFT_LARGE_ONLY" in env), ("HIPSOXR_FFT_SMALL_ONLY" in env), ("HIPSOXR_FFT_NO_TINY" in env)
    force_k = int(env.get("HIPSOXR_DEBUG_FFT_K", 0))
    big = sml = tiny = None
    for r in ratio_rows:
        if r["small"] == 3:
            continue
        if r["small"] == 2:
            tiny = r
        elif r["small"]:
            sml = r
        else:
            big = r

    def ok(r):
        return hop_out(r["L"], r["M"], T, r["k"]) > 0

    if big is None or not ok(big):
        return None
    use = big
    if sml is not None and ((not large) or small_only or wide) and ok(sml):    # (wgs < 480 && !large_only) || small_only || f64
        use = sml
    if use is sml and tiny is not None and not large and not no_tiny and ok(tiny):   # f64 || wgs <= 500
        use = tiny
    if f32_unit and force_k > 0:
        pick = None
        for r in ratio_rows:
            if r["k"] == force_k and ("pair2", "f32") in instances_of(r, macros):
                pick = r
        if pick is not None and ok(pick):
            use = pick
    return use


# Instances that no job reaches, under any switch: (row, instance) -> the host condition that bars it.  Everything else in
# the table must get a case from case_plan (tests/test_fft_table.py).
_FULL_SIZE_ROWS_OF_RATIOS_WITH_A_HALF_SIZE_ROW = ((147, 160, 32, 0), (160, 147, 32, 0), (160, 441, 16, 0), (441, 160, 16, 0),
                                                  (1, 2, 2048, 0), (2, 1, 2048, 0), (1, 3, 1792, 0), (3, 1, 1792, 0),
                                                  (2, 3, 1792, 0), (3, 2, 1792, 0))
UNREACHABLE = {(row, inst): "float64 arithmetic never stays on the full-size row of a ratio that has a half-size one: "
                            "`(...) || switches().fft_small_only || v.f64` in fft_choose_row takes `sml` whenever its geometry "
                            "is admissible (gs.ok), HIPSOXR_FFT_LARGE_ONLY set or not"
               for row in _FULL_SIZE_ROWS_OF_RATIOS_WITH_A_HALF_SIZE_ROW for inst in INSTANCES if inst[1] in WIDE_KINDS}


def case_plan(rows, macros, taps_of, half=None):
    """taps_of(L, M, quality) -> taps per phase.  -> (cases, status): cases = dicts child, row, form, kind, quality, hop;
    status[(row key, instance, quality)] = "case" | "inadmissible" | "unreachable".  half (parse_half): the plan of the
    float16 / bfloat16 instances instead — a half job takes the row the float32 job of its shape takes, on float32
    arithmetic, under the same switches and in children of the same names."""
    envs = children(rows)
    cases, status = [], {}
    for r in rows:
        ratio = [x for x in rows if (x["L"], x["M"]) == (r["L"], r["M"])]
        for q in QUALITIES:
            T = taps_of(r["L"], r["M"], q)
            hop = hop_out(r["L"], r["M"], T, r["k"])
            for inst in (instances_of(r, macros) if half is None else half_instances_of(r, half)):
                key = (row_key(r), inst, q)
                if not hop or pick_row(ratio, T, {}, False, False, macros) is None:
                    status[key] = "inadmissible"     # (fft_geometry: g.ok == false for the row, or for the ratio's full-size row)
                    continue
                status[key] = "unreachable"
                for name, env in envs.items():
                    if pick_row(ratio, T, env, inst[1] in WIDE_KINDS, inst in F32_UNIT, macros) is r:
                        status[key] = "case"
                        cases.append(dict(child=name, row=row_key(r), form=inst[0], kind=inst[1], quality=q, hop=hop))
                        break
    return cases, status


def case_id(c):
    return "%d:%d:k%d:s%d/%s/%s/%s" % (c["row"] + (c["form"], c["kind"], c["quality"]))


# ---------------------------------------------------------------------------------------------------------------------
# jobs of a case: output lengths around the seams of its work items, layouts of its form, inputs
LAYOUTS = {"pair2": ("col", "batch3"), "strided2_cp": ("pair", "pair4x2"), "strided2_st": ("odd3", "slice")}
SHAPES = {"col": (1, 1), "batch3": (3, 1), "pair": (1, 2), "pair4x2": (2, 4), "odd3": (1, 3), "slice": (1, 1)}   # clips, channels


def shortest_in(out_len, t, L, M):
    """The shortest input with at least t outputs."""
    n = max(1, t * M // L)
    while out_len(n) < t:
        n += 1
    while n > 1 and out_len(n - 1) >= t:
        n -= 1
    return n


def out_lengths(c, out_len):
    """-> [(n_out, n_in)].  Work item = a pair of blocks (pair2, strided2_st) or one block (strided2_cp): lengths that end
    one output before, on and one behind the kept run of one item (and of two, for single blocks), an odd block count
    (3 hop + 5: the last pair has no partner), and several items with a seeded remainder.  An up-sampling ratio steps over
    some lengths: there the nearest attainable length on the same side of the seam stands in (the last one not behind
    it, the first one behind it); "on" is kept where it is attainable."""
    h, L, M = c["hop"], c["row"][0], c["row"][1]
    r = int(np.random.default_rng(list(c["row"]) + [QUALITIES.index(c["quality"])]).integers(1, h))
    seams = ([h] if c["form"] == "strided2_cp" else []) + [2 * h]
    got = []

    def add(n_in):
        if n_in >= 1 and out_len(n_in) >= 1 and (out_len(n_in), n_in) not in got:
            got.append((out_len(n_in), n_in))

    for s in seams:
        n = shortest_in(out_len, s, L, M)
        if out_len(n) == s:
            add(n - 1)                  # ... the last length before the seam's end,
            add(n)                      # on it,
            m = n + 1
            while out_len(m) == s:
                m += 1
            add(m)                      # and the first length behind it
        else:
            add(n - 1)
            add(n)
    for t in (3 * h + 5, 7 * h + r):
        add(shortest_in(out_len, t, L, M))
    return got


_master = {}


def master(L, M, n_in, col):
    """float64 Gaussian at level 0.25: one signal per (ratio, length), another seed per column."""
    key = (L, M, n_in, col)
    if key not in _master:
        if len(_master) > 4096:
            _master.clear()
        _master[key] = np.random.default_rng([L, M, n_in, col]).standard_normal(n_in) * 0.25
    return _master[key]


def cast(x64, kind):
    """The master signal as the samples of a kind (levels of tests/test_gpu_fft_pcm.py: int16 RMS 5000, int32 RMS 2^27)."""
    if kind in ("f32", "f32on64"):
        return x64.astype(np.float32)
    if kind == "f64":
        return x64
    if kind == "i16":
        return np.clip(np.rint(x64 * (5000 / 0.25)), -32768, 32767).astype(np.int16)
    return np.clip(np.rint(x64 * (2.0 ** 27 / 0.25)), -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int32)


def rms(a):
    return float(np.sqrt(np.mean(np.asarray(a, np.float64) ** 2))) if np.size(a) else 0.0


def stretch_rms(err, n=2048):
    """RMS of every whole stretch of n samples (of the whole signal where it is shorter)."""
    err = np.asarray(err, np.float64)
    if len(err) < n:
        return np.array([rms(err)])
    return np.sqrt(np.mean(err[:len(err) // n * n].reshape(-1, n) ** 2, axis=1))


_refs = {}


def oracle_ref(o, L, M, quality, x, key):
    """The oracle's float64 direct form on its own bank, cached per (ratio, quality, length, column, cast)."""
    key = (L, M, quality) + key
    if key not in _refs:
        if len(_refs) > 4096:
            _refs.clear()
        fi, fo = rates_of(L, M)
        _refs[key] = o.resample(np.asarray(x, np.float64), fi, fo, quality, mode="ref")
    return _refs[key]


# ---------------------------------------------------------------------------------------------------------------------
# the float64 overlap-save model at a row's block size against the direct form: what the METHOD leaves at that k
def model_floor(o, ovs, row, quality):
    """-> dict rel, stretch, point (each relative to rms(ref), the maximum over the float64 inputs of every form's jobs),
    or None where the row is not admissible for the recipe."""
    L, M, k, _ = row
    fi, fo = rates_of(L, M)
    pl = o.plan(fi, fo, quality)
    assert (pl.L, pl.M) == (L, M)
    hop = hop_out(L, M, pl.T, k)
    if not hop:
        return None
    fp = ovs.Plan(pl, periods=k)
    assert fp.hop * L == hop, (row, fp.hop * L, hop)
    worst = dict(rel=0.0, stretch=0.0, point=0.0)
    seen = set()
    for form in LAYOUTS:
        c = dict(row=row, form=form, quality=quality, hop=hop)
        ncols = max(SHAPES[l][0] * SHAPES[l][1] for l in LAYOUTS[form])
        for n_out, n_in in out_lengths(c, pl.out_len):
            for col in range(ncols):
                if (n_in, col) in seen:
                    continue
                seen.add((n_in, col))
                x = master(L, M, n_in, col)
                ref = oracle_ref(o, L, M, quality, x, (n_in, col, "f64"))
                err = ovs.resample(fp, x, out_len=len(ref)) - ref
                s = rms(ref)
                worst["rel"] = max(worst["rel"], rms(err) / s)
                worst["stretch"] = max(worst["stretch"], float(stretch_rms(err).max()) / s)
                worst["point"] = max(worst["point"], float(np.abs(err).max()) / s)
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# the child process
WHOLE_BAR = {"f64": {"VHQ": 2e-9, "HQ": 1e-6}, "f32on64": {"VHQ": 5e-8, "HQ": 1e-6}}   # tests/test_gpu_fft.py
SENT = 77
PAD = 8


class LogTail:
    def __init__(self, path):
        self.path, self.pos = path, 0

    def take(self):
        if not os.path.exists(self.path):
            return []
        with open(self.path) as f:
            f.seek(self.pos)
            text = f.read()
            self.pos = f.tell()
        return [dict(kv.split("=", 1) for kv in line.split()) for line in text.splitlines() if line.strip()]


def _run_child(name):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "python-soxr_amd"))
    import torch
    from soxr_amd import device as dev
    from oracle import oracle as o
    o.lib()
    with open(FLOOR_JSON) as f:
        floor = json.load(f)["floor"]
    log = LogTail(os.environ["HIPSOXR_DEBUG_LAUNCH_LOG"])
    rows, macros = parse_table()
    plans = {}

    def plan_of(L, M, q):
        if (L, M, q) not in plans:
            plans[(L, M, q)] = dev.Plan(*rates_of(L, M), q)
            assert (plans[(L, M, q)].L, plans[(L, M, q)].M) == (L, M)
        return plans[(L, M, q)]

    cases, _ = case_plan(rows, macros, lambda L, M, q: plan_of(L, M, q).taps)
    results = {}

    def buffers(layout, x_cols, n_out, tdtype):
        """-> input tensor, padded output buffer, the index of the result inside it.  x_cols: numpy columns, clip-major."""
        clips, ch = SHAPES[layout]
        x = np.stack(x_cols).reshape(clips, ch, -1).transpose(0, 2, 1)           # [clips, frames, channels]
        if layout == "col":
            return torch.from_numpy(np.ascontiguousarray(x[0, :, 0])).cuda(), torch.empty(n_out + 2 * PAD, dtype=tdtype, device="cuda"), (slice(PAD, PAD + n_out),)
        if layout == "slice":                                                      # channel 1 of 4: frame stride 4 in and out
            wide = np.random.default_rng(len(x_cols[0])).standard_normal((x.shape[1], 4)) * 0.25
            wide = cast(wide.reshape(-1), {torch.float32: "f32", torch.float64: "f64"}[tdtype]).reshape(-1, 4).copy()
            wide[:, 1] = x[0, :, 0]
            return torch.from_numpy(wide).cuda()[:, 1], torch.empty((n_out + 2 * PAD, 4), dtype=tdtype, device="cuda"), (slice(PAD, PAD + n_out), 1)
        if clips == 1:
            return torch.from_numpy(np.ascontiguousarray(x[0])).cuda(), torch.empty((n_out + 2 * PAD, ch), dtype=tdtype, device="cuda"), (slice(PAD, PAD + n_out),)
        return (torch.from_numpy(np.ascontiguousarray(x)).cuda(), torch.empty((clips, n_out + 2 * PAD, ch), dtype=tdtype, device="cuda"),
                (slice(None), slice(PAD, PAD + n_out)))

    def launch(plan, xt, buf, idx, kernel, **kw):
        """One job into the padded buffer -> (result as [columns, frames] numpy, sentinels intact, log lines)."""
        buf.fill_(SENT)
        log.take()
        dev.resample_tensor(plan, xt, out=buf[idx], kernel=kernel, **kw)
        torch.cuda.synchronize()
        lines = log.take()
        b = buf.cpu().numpy()
        y = b[idx]
        outside = b.copy()
        outside[idx] = SENT
        y3 = y[None, :, None] if y.ndim == 1 else (y[None] if y.ndim == 2 else y)
        return np.ascontiguousarray(y3.transpose(0, 2, 1).reshape(-1, y3.shape[1])), bool((outside == SENT).all()), lines

    for c in cases:
        if c["child"] != name:
            continue
        cid = case_id(c)
        print("TABLE_CASE", cid, flush=True)
        L, M, k, small = c["row"]
        q, kind, form = c["quality"], c["kind"], c["form"]
        plan = plan_of(L, M, q)
        fails, figs, jobs = [], {}, 0
        want = dict(form=form, L=str(L), M=str(M), k=str(k), small=str(small), kind=kind, hop_out=str(c["hop"]), window="0")

        def check_line(lines, want, tag):
            if len(lines) != 1:
                fails.append(f"{tag}: {len(lines)} launch log lines: {lines}")
                return False
            bad = {f: (lines[0].get(f), v) for f, v in want.items() if lines[0].get(f) != v}
            if bad:
                fails.append(f"{tag}: served by {lines[0]} — (got, wanted) {bad}")
            return not bad

        def fig(nm, v, bar, tag):
            figs[nm] = max(figs.get(nm, 0.0), v / bar)
            if not v <= bar:
                fails.append(f"{tag}: {nm} {v:.4g} > {bar:.4g}")

        tdtype = {"f32": torch.float32, "f32on64": torch.float32, "f64": torch.float64, "i16": torch.int16, "i32": torch.int32}[kind]
        kernel = {"f32": FFT, "f64": FFT, "f32on64": FFT_F64, "i16": FFT_PCM, "i32": FFT_PCM}[kind]
        for n_out, n_in in out_lengths(c, plan.out_len):
            for layout in LAYOUTS[form]:
                tag = f"n_out={n_out} {layout}"
                jobs += 1
                ncols = SHAPES[layout][0] * SHAPES[layout][1]
                x64 = [master(L, M, n_in, col) for col in range(ncols)]
                try:
                    xt, buf, idx = buffers(layout, [cast(x, kind) for x in x64], n_out, tdtype)
                    kw = dict(dither=True, dither_seed=7, clip_counter=torch.zeros(1, dtype=torch.int64, device="cuda")) if kind in ("i16", "i32") else {}
                    y, intact, lines = launch(plan, xt, buf, idx, kernel, **kw)
                    n_clip = int(kw["clip_counter"].item()) if kw else 0
                    if kw:
                        kw["clip_counter"].zero_()
                    y2, intact2, _ = launch(plan, xt, buf, idx, kernel, **kw)
                except RuntimeError as e:
                    fails.append(f"{tag}: {e}; launch log: {log.take()}")
                    continue
                check_line(lines, want, tag)
                if y.shape != (ncols, n_out):
                    fails.append(f"{tag}: result shape {y.shape}")
                    continue
                if not (intact and intact2):
                    fails.append(f"{tag}: a sentinel beside the result was overwritten")
                if y.tobytes() != y2.tobytes():
                    fails.append(f"{tag}: two runs of the job differ")
                if kind in ("i16", "i32"):
                    # == the float job of the same arithmetic width, row and layout + the host restatement of the output stage
                    fk = "f32" if kind == "i16" else "f64"
                    fdt = torch.float32 if kind == "i16" else torch.float64
                    xf, fbuf, fidx = buffers(layout, [cast(x, kind).astype(np.float32 if kind == "i16" else np.float64) for x in x64], n_out, fdt)
                    yf, _, flines = launch(plan, xf, fbuf, fidx, FFT)
                    check_line(flines, dict(want, kind=fk), tag + " (float job)")
                    clips = 0
                    for col in range(ncols):
                        wantq, nc = o.quantize(yf[col], cast(x64[0], kind).dtype, channel=col % SHAPES[layout][1], k0=0, dither=True, seed=7)
                        clips += nc
                        nd = int(np.count_nonzero(wantq != y[col]))
                        if nd:
                            fails.append(f"{tag} column {col}: {nd} of {n_out} samples differ from the float job + quantize")
                    if clips != n_clip:
                        fails.append(f"{tag}: clip count {n_clip}, host {clips}")
                    continue
                for col in range(ncols):
                    xin = cast(x64[col], kind)
                    ref = oracle_ref(o, L, M, q, xin, (n_in, col, "f64" if kind == "f64" else "f32"))
                    if ref.shape != (n_out,):
                        fails.append(f"{tag}: oracle length {ref.shape}")
                        continue
                    err = y[col].astype(np.float64) - ref
                    s = rms(ref)
                    t2 = f"{tag} column {col}"
                    if kind == "f32":                                              # the bars of tests/test_gpu_fft.py
                        fig("rel_rms", rms(err) / s, 1e-6, t2)
                        fig("max_err", float(np.abs(err).max()), 4e-5 * s, t2)
                        fig("stretch", float(stretch_rms(err).max()), 4e-6 * s, t2)
                        fig("ends", float(max(np.abs(err[:500]).max(), np.abs(err[-500:]).max())), 1e-5, t2)
                    else:
                        fl = floor[row_name(dict(L=L, M=M, k=k, small=small))][q]
                        # (float32 results of float64 arithmetic: + the rounding of the result, <= 2^-24 of the sample)
                        r24 = 2.0 ** -24 if kind == "f32on64" else 0.0
                        fig("rel_rms", rms(err) / s, WHOLE_BAR[kind][q], t2)
                        fig("stretch", float(stretch_rms(err).max()), 4 * fl["stretch"] * s + r24 * float(stretch_rms(ref).max()), t2)
                        fig("point", float(np.abs(err).max()), 4 * fl["point"] * s + r24 * float(np.abs(ref).max()), t2)
        results[cid] = dict(ok=not fails, jobs=jobs, fails=fails[:6], n_fails=len(fails), share_of_bar={k_: round(v, 4) for k_, v in figs.items()})
        print("TABLE_RESULT", cid, json.dumps(results[cid]), flush=True)
    print("TABLE_PROBE " + json.dumps(results))


# ---------------------------------------------------------------------------------------------------------------------
# the child process of the float16 / bfloat16 instances (tests/test_gpu_fft_table_half.py)
# pair2: col_odd = the input is base[1:] (2-byte aligned only), the output starts at element PAD + 1; col_o6 = aligned
# input, output at PAD + 6 (4-byte aligned, inside a 16-byte granule) — hop_out is even, so with a granule-aligned output
# the store loop would never meet an odd shift.  strided2_cp: pair_o1f = input and output one frame in (4-byte, not 8-byte
# aligned: still one aligned word per frame, still fused).
HALF_LAYOUTS = {"pair2": ("col", "batch3", "col_odd", "col_o6"), "strided2_cp": ("pair", "pair4x2", "pair_o1f")}
HALF_SHAPES = dict(SHAPES, col_odd=(1, 1), col_o6=(1, 1), pair_o1f=(1, 2))
HALF_OFFSETS = {"col_odd": (1, PAD + 1, 8), "col_o6": (0, PAD + 6, 8), "pair_o1f": (1, PAD + 1, 2)}   # frames: input, output, longer buffer
HALF_FORMAT = {"f16": (10, -14), "bf16": (7, -126)}     # stored significand bits, exponent of the smallest normal
SUBNORMAL_SCALE = 2.0 ** -12                            # float16, column 2 of batch3: RMS 2^-14, the smallest normal


def half_ulp(y, kind):
    """Half the spacing of the half type at |y| (float64): subnormal spacing below the smallest normal."""
    bits, emin = HALF_FORMAT[kind]
    e = np.floor(np.log2(np.maximum(np.abs(y), 2.0 ** emin)))
    return 0.5 * 2.0 ** (e - bits)


def half_bar(ref, kind):
    """Pointwise bar of a half result against the float64 direct form: the float32 engine's own (4e-5 x RMS,
    tests/test_gpu_fft.py) plus the one rounding, at the largest magnitude the float32 value can have."""
    s = 4e-5 * rms(ref)
    return s + half_ulp(np.abs(ref) + s, kind)


def _run_half_child(name):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "python-soxr_amd"))
    import ctypes as C
    import torch
    torch.cuda.init()
    torch.zeros(1, device="cuda").cpu()
    from soxr_amd import _native as nat, device as dev
    from oracle import oracle as o
    o.lib()
    log = LogTail(os.environ["HIPSOXR_DEBUG_LAUNCH_LOG"])
    rows, macros = parse_table()
    half = parse_half()
    plans = {}

    def plan_of(L, M, q):
        if (L, M, q) not in plans:
            plans[(L, M, q)] = dev.Plan(*rates_of(L, M), q)
            assert (plans[(L, M, q)].L, plans[(L, M, q)].M) == (L, M)
        return plans[(L, M, q)]

    cases, _ = case_plan(rows, macros, lambda L, M, q: plan_of(L, M, q).taps, half=half)
    results = {}
    tdt = {"f16": torch.float16, "bf16": torch.bfloat16}

    def bits(t):
        return t.contiguous().view(torch.int16)

    def buffers(layout, cols, n_out):
        """cols: the columns as host tensors of the half type, clip-major.  -> the base tensor of the input (host), the
        frame its view starts at, the shape of the padded output buffer, the index of the result inside it."""
        clips, ch = HALF_SHAPES[layout]
        x = torch.stack(cols).reshape(clips, ch, -1).permute(0, 2, 1).contiguous()   # [clips, frames, channels]
        i_off, o_off, more = HALF_OFFSETS.get(layout, (0, PAD, 0))
        idx = (slice(o_off, o_off + n_out),)
        if ch == 1 and clips == 1:
            base, shape = x[0, :, 0], (n_out + 2 * PAD + more,)
        elif clips == 1:
            base, shape = x[0], (n_out + 2 * PAD + more, ch)
        else:
            base, shape, idx = x, (clips, n_out + 2 * PAD, ch), (slice(None),) + idx
        if i_off:
            base = torch.cat([torch.zeros_like(base[:i_off]), base])
        return base.contiguous(), i_off, shape, idx

    def launch(plan, xt, buf, idx):
        """One job into the padded buffer -> (result as [columns, frames] host tensor, sentinels intact, log lines)."""
        buf.fill_(SENT)
        log.take()
        dev.resample_tensor(plan, xt, out=buf[idx], kernel=FFT)
        torch.cuda.synchronize()
        lines = log.take()
        b = buf.cpu()
        y = b[idx]
        outside = b.clone()
        outside[idx] = SENT
        y3 = y[None, :, None] if y.ndim == 1 else (y[None] if y.ndim == 2 else y)
        return y3.permute(0, 2, 1).reshape(-1, y3.shape[1]).contiguous(), bool((outside == SENT).all()), lines

    def raw_ragged(plan, dtype, x, out, table):
        j = nat.Job()
        j.in_, j.out, j.elem, j.kernel = x.data_ptr(), out.data_ptr(), dev._torch_elem(dtype), FFT
        j.n_clips, j.n_channels = table.shape[0], 1
        j.in_frame_stride, j.in_chan_stride, j.out_frame_stride, j.out_chan_stride = 1, 1, 1, 1
        j.in_frames, j.out_frames = int(table[:, 1].max()), int(table[:, 3].max())
        j.clip_table = table.ctypes.data
        nat.check(nat.lib.hipsoxr_run_device(plan.handle, C.byref(j), torch.cuda.current_stream().cuda_stream))

    for c in cases:
        if c["child"] != name:
            continue
        cid = case_id(c)
        print("TABLE_CASE", cid, flush=True)
        L, M, k, small = c["row"]
        q, kind, form = c["quality"], c["kind"], c["form"]
        dt = tdt[kind]
        plan = plan_of(L, M, q)
        fails, figs, jobs = [], {}, 0
        want = dict(form=form, L=str(L), M=str(M), k=str(k), small=str(small), kind=kind, hop_out=str(c["hop"]), window="0")

        def check_line(lines, want, tag):
            if len(lines) != 1:
                fails.append(f"{tag}: {len(lines)} launch log lines: {lines}")
                return
            bad = {f: (lines[0].get(f), v) for f, v in want.items() if lines[0].get(f) != v}
            if bad:
                fails.append(f"{tag}: served by {lines[0]} — (got, wanted) {bad}")

        def signal(n_in, col, scale=1.0):
            """The master Gaussian (x scale, a power of two), rounded to the half type: a host tensor."""
            return torch.from_numpy(master(L, M, n_in, col) * scale).to(dt)

        def identity(yh, yf, tag):
            """half result == float32 twin rounded once, bit for bit"""
            diff = (bits(yh) != bits(yf.to(dt))).reshape(-1)
            if bool(diff.any()):
                at = int(diff.nonzero()[0])
                fails.append(f"{tag}: {int(diff.sum())} of {diff.numel()} elements differ from the float32 twin rounded once, the first at {at}")

        def oracle_bar(yh, xh, key, n_out, tag, subnormal=False):
            """every point of a column against the float64 direct form on the widened input"""
            ref = oracle_ref(o, L, M, q, xh.double().numpy(), key + (kind,))
            if ref.shape != (n_out,):
                fails.append(f"{tag}: oracle length {ref.shape}")
                return
            if subnormal:
                n_sub = int(np.count_nonzero((np.abs(ref) > 0) & (np.abs(ref) < 2.0 ** -14)))
                if not n_sub > n_out / 10:
                    fails.append(f"{tag}: the subnormal column is vacuous: {n_sub} of {n_out} reference outputs in (0, 2^-14)")
            share = float((np.abs(yh.double().numpy() - ref) / half_bar(ref, kind)).max())
            figs["oracle"] = max(figs.get("oracle", 0.0), share)
            if not share <= 1.0:
                fails.append(f"{tag}: |y - ref| reaches {share:.4g} of 4e-5 x RMS + half an ulp")

        for n_out, n_in in out_lengths(c, plan.out_len):
            for layout in HALF_LAYOUTS[form]:
                tag = f"n_out={n_out} {layout}"
                jobs += 1
                ncols = HALF_SHAPES[layout][0] * HALF_SHAPES[layout][1]
                sub = {2} if (kind == "f16" and layout == "batch3") else set()
                cols = [signal(n_in, col, SUBNORMAL_SCALE if col in sub else 1.0) for col in range(ncols)]
                try:
                    base, i_off, shape, idx = buffers(layout, cols, n_out)
                    xh = base.cuda()
                    xf = xh.float()
                    bufh, buff = torch.empty(shape, dtype=dt, device="cuda"), torch.empty(shape, dtype=torch.float32, device="cuda")
                    yh, intact, lines = launch(plan, xh[i_off:], bufh, idx)
                    if layout == HALF_LAYOUTS[form][0]:
                        yh2, intact2, _ = launch(plan, xh[i_off:], bufh, idx)
                        if not torch.equal(bits(yh), bits(yh2)):
                            fails.append(f"{tag}: two runs of the job differ")
                        intact = intact and intact2
                    yf, intactf, flines = launch(plan, xf[i_off:], buff, idx)
                except RuntimeError as e:
                    fails.append(f"{tag}: {e}; launch log: {log.take()}")
                    continue
                check_line(lines, want, tag)
                check_line(flines, dict(want, kind="f32"), tag + " (float32 twin)")
                if tuple(yh.shape) != (ncols, n_out) or yf.shape != yh.shape:
                    fails.append(f"{tag}: result shape {tuple(yh.shape)}, twin {tuple(yf.shape)}")
                    continue
                if not (intact and intactf):
                    fails.append(f"{tag}: a sentinel beside the result was overwritten")
                identity(yh, yf, tag)
                for col in range(ncols):
                    oracle_bar(yh[col], cols[col], (n_in, "2s" if col in sub else col), n_out, f"{tag} column {col}", col in sub)

        if form == "pair2":
            # one ragged job (a clip table): the 3 hop + 5 input, one frame short of the two-item seam, 1 frame and none,
            # packed at odd element offsets, guard elements between the outputs
            tag = "ragged"
            jobs += 1
            h = c["hop"]
            frames = [shortest_in(plan.out_len, 3 * h + 5, L, M), shortest_in(plan.out_len, 2 * h, L, M) - 1, 1, 0]
            n_outs = [plan.out_len(n) for n in frames]
            in_off, out_off, pos_i, pos_o = [], [], 1, PAD + 1
            for n, m in zip(frames, n_outs):
                in_off.append(pos_i)
                out_off.append(pos_o)
                pos_i += n + (1 if (pos_i + n) % 2 == 0 else 2)           # the next clip starts at an odd element again
                pos_o += m + (PAD + 1 if (pos_o + m + PAD + 1) % 2 else PAD)
            assert all(v % 2 for v in in_off + out_off)
            table = np.ascontiguousarray(np.stack([in_off, frames, out_off, n_outs], axis=1), dtype=np.int64)
            clips = [signal(n, 0) for n in frames]
            x = torch.zeros(pos_i + PAD, dtype=dt)
            for a, n, s in zip(in_off, frames, clips):
                x[a:a + n] = s
            try:
                xh = x.cuda()
                outh = torch.full((pos_o + PAD,), float(SENT), dtype=dt, device="cuda")
                outf = torch.full((pos_o + PAD,), float(SENT), dtype=torch.float32, device="cuda")
                log.take()
                raw_ragged(plan, dt, xh, outh, table)
                torch.cuda.synchronize()
                lines = log.take()
                raw_ragged(plan, torch.float32, xh.float(), outf, table)
                torch.cuda.synchronize()
                flines = log.take()
                check_line(lines, dict(want, ragged="4"), tag)
                check_line(flines, dict(want, kind="f32", ragged="4"), tag + " (float32 twin)")
                yh, yf = outh.cpu(), outf.cpu()
                identity(yh, yf, tag)                                      # (77 is exact in all three types: the guards compare too)
                guard = torch.ones(yh.shape[0], dtype=torch.bool)
                for a, m in zip(out_off, n_outs):
                    guard[a:a + m] = False
                if not bool((yh[guard] == SENT).all() and (yf[guard] == SENT).all()):
                    fails.append(f"{tag}: guard elements between packed clips were written")
                for i, (a, m, n) in enumerate(zip(out_off, n_outs, frames)):
                    if m:
                        oracle_bar(yh[a:a + m], clips[i], (n, 0), m, f"{tag} clip {i}")
            except RuntimeError as e:
                fails.append(f"{tag}: {e}; launch log: {log.take()}")

        results[cid] = dict(ok=not fails, jobs=jobs, fails=fails[:6], n_fails=len(fails), share_of_bar={k_: round(v, 4) for k_, v in figs.items()})
        print("TABLE_RESULT", cid, json.dumps(results[cid]), flush=True)
    print("TABLE_PROBE " + json.dumps(results))


if __name__ == "__main__":
    if sys.argv[1].startswith("half:"):
        _run_half_child(sys.argv[1][len("half:"):])
    else:
        _run_child(sys.argv[1])
