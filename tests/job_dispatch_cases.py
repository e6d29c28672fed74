"""The jobs of tests/test_gpu_job_dispatch.py — one list, read by the probe that runs them (tests/_job_dispatch_probe.py), by
the generator of the fixture (tests/golden/make_job_dispatch_golden.py) and by the test module.  No torch, no library here.

A case: name, env ("default" | "no_fft" | "no_two_stage": the child process it runs in), plan (EXACT_PLAN: an HQ exact-bank
plan; INTERP_PLAN: an HQ interpolated-phase plan), dtype, kernel, and either
    shape = [clips, out_frames, channels]  an equal-length job of exactly out_frames outputs per column (in_frames: the least
                                           count that yields them; "in_frames": given outright instead, every output taken)
    table = [out_frames per clip]          a clip table, packed interleaved clips, rows made the same way
plus in_abs0 / out_k0, dither, and for a table one defect: "bad" = [clip, field, value] written into the row ("plan+1": one
more than the plan's output length of the row's input), "job_in" / "job_out" = what the job says instead of the largest row.
Sizes: the least at which a decision can flip — the AUTO rule is 2^13 outputs in all."""

AUTO, GATHER, FFT, EXACT, WAVE_DOT, FFT_F64, FFT_PCM = 0, 1, 5, 6, 7, 8, 9
EXACT_PLAN = (48000, 44100, "HQ")
INTERP_PLAN = (48000, 44101, "HQ")
ENVS = {"default": {}, "no_fft": {"HIPSOXR_NO_FFT": "1"}, "no_two_stage": {"HIPSOXR_NO_TWO_STAGE": "1"}}
N = 1 << 13
FOLD = "fold_65536x2x4_i16_dither"


def _cases():
    c = []

    def add(name, env="default", plan=EXACT_PLAN, dtype="f32", kernel=AUTO, **kw):
        c.append(dict(name=name, env=env, plan=list(plan), dtype=dtype, kernel=kernel, **kw))

    # ---- around the AUTO threshold: totals 2^13 - 1 / 2^13 mono, 2 x 4095 / 2 x 4096 stereo (an odd total has no stereo job)
    for dt in ("f32", "f64", "i16", "f16"):
        add(f"mono_{dt}_below", dtype=dt, shape=[1, N - 1, 1])
        add(f"mono_{dt}_at", dtype=dt, shape=[1, N, 1])
        add(f"stereo_{dt}_below", dtype=dt, shape=[1, N // 2 - 1, 2])
        add(f"stereo_{dt}_at", dtype=dt, shape=[1, N // 2, 2])
        add(f"table_{dt}_below", dtype=dt, table=[4000, 4000, 191], ch=1)
        add(f"table_{dt}_at", dtype=dt, table=[4000, 4000, 192], ch=1)
    add("table_stereo_f32_below", table=[2000, 2000, 95], ch=2)
    add("table_stereo_f32_at", table=[2000, 2000, 96], ch=2)
    add("mono_f32_below_fft", kernel=FFT, shape=[1, N - 1, 1])
    add("table_f32_below_fft", kernel=FFT, table=[4000, 4000, 191], ch=1)
    for dt in ("f32", "f16"):  # HIPSOXR_NO_FFT: AUTO stays exact at any size
        add(f"nofft_mono_{dt}_at", env="no_fft", dtype=dt, shape=[1, N, 1])
        add(f"nofft_table_{dt}_at", env="no_fft", dtype=dt, table=[4000, 4000, 192], ch=1)
    add("nofft_mono_f32_fft", env="no_fft", kernel=FFT, shape=[1, N, 1])  # (by name: the switch speaks of AUTO alone)
    # ---- selector refusals
    add("pcm_on_float", kernel=FFT_PCM, shape=[1, N, 1])
    add("pcm_window", dtype="i16", kernel=FFT_PCM, shape=[1, N, 1], out_k0=5)
    add("pcm_served", dtype="i16", kernel=FFT_PCM, shape=[1, N, 1])
    add("f64_on_half", dtype="f16", kernel=FFT_F64, shape=[1, N, 1])
    add("wave_dot_on_half", dtype="f16", kernel=WAVE_DOT, shape=[1, 600, 1])
    # ---- interpolated-phase plan: the two-stage form
    # (it admits a signal of 8192 frames on its shorter side — here the output's: the plan resamples down)
    for frames in (N - 1, N):
        add(f"interp_{frames}_auto", plan=INTERP_PLAN, shape=[1, frames, 1])
        add(f"interp_{frames}_fft", plan=INTERP_PLAN, kernel=FFT, shape=[1, frames, 1])
    add("interp_table_auto", plan=INTERP_PLAN, table=[9000, 500, 10000], ch=1)  # two long clips and a short one
    add("interp_table_no_two_stage", env="no_two_stage", plan=INTERP_PLAN, table=[9000, 500, 10000], ch=1)
    add("interp_8192_no_two_stage", env="no_two_stage", plan=INTERP_PLAN, shape=[1, N, 1])
    add("interp_8192_fft_no_two_stage", env="no_two_stage", plan=INTERP_PLAN, kernel=FFT, shape=[1, N, 1])
    add("interp_8192_no_fft", env="no_fft", plan=INTERP_PLAN, shape=[1, N, 1])
    add("interp_8192_fft_no_fft", env="no_fft", plan=INTERP_PLAN, kernel=FFT, shape=[1, N, 1])  # (by name: HIPSOXR_NO_FFT speaks of AUTO alone)
    add("interp_table_no_fft", env="no_fft", plan=INTERP_PLAN, table=[9000, 500, 10000], ch=1)
    # ---- tables: refusals and the clip loop
    add("table_window", table=[300, 200, 100], ch=1, in_abs0=3)
    add("row_neg_in_offset", table=[300, 200, 100], ch=1, bad=[1, 0, -1])
    add("row_neg_in_frames", table=[300, 200, 100], ch=1, bad=[1, 1, -1])
    add("row_neg_out_offset", table=[300, 200, 100], ch=1, bad=[1, 2, -1])
    add("row_neg_out_frames", table=[300, 200, 100], ch=1, bad=[1, 3, -1])
    add("row_in_above_job", table=[300, 200, 100], ch=1, job_in=-1)
    add("row_out_above_job", table=[300, 200, 100], ch=1, job_out=-1)
    add("row_out_above_plan", table=[300, 200, 100], ch=1, bad=[2, 3, "plan+1"], job_out=+1)
    add("table_wave_dot", kernel=WAVE_DOT, table=[300, 0, 100], ch=1)  # the clip loop (k_wave_dot writes no log line: the values say it ran)
    add("table_f16_clip_loop", dtype="f16", table=[4000, 0, 4000], ch=1)  # ... one line per non-empty clip: each a plain half job
    add("table_wave_dot_all_empty", kernel=WAVE_DOT, table=[0, 0], ch=1)
    # ---- the fold with both axes wide: clip ranges, the first folded again over its channels
    add(FOLD, dtype="i16", kernel=EXACT, shape=[65536, 0, 2], in_frames=4, dither=True, same_channels=True,
        cut=[[0, 30000], [30000, 60000], [60000, 65535], [65535, 65536]])
    add("fold_65536ch_f32", kernel=EXACT, shape=[1, 0, 65536], in_frames=4)
    return c


CASES = _cases()
assert len({c["name"] for c in CASES}) == len(CASES)


def summarize(log_text):
    """A launch log's lines as the fixture holds them: the kernel's name (the frequency-domain engine's lines carry form= and
    kind= instead of kernel=), and the column and clip-table counts where the line has them."""
    lines = []
    for ln in log_text.splitlines():
        f = dict(tok.split("=", 1) for tok in ln.split() if "=" in tok)
        if not f:
            continue
        rec = {"kernel": f["kernel"] if "kernel" in f else "fft:" + f.get("form", "?")}
        for key in ("cols", "ragged"):
            if key in f:
                rec[key] = int(f[key])
        lines.append(rec)
    return lines
