"""Helper of tests/test_gpu_fft_forms.py: the launch forms of the frequency-domain engine (csrc/fft.hip, launch_fft_impl)
that tests/test_gpu_fft_table.py does not see — window jobs (stream chunks), ragged batches, the wave form, k_fft_block,
"none", the two-stage form's inner calls — plus one small job of every instance kind, under the process's HIPSOXR_*
environment with the debug-switch build's launch log (HIPSOXR_DEBUG_LAUNCH_LOG).

argv[1] names the child: "plain" (HIPSOXR_FFT_NO_WAVE and HIPSOXR_DEBUG_WAVE_MIN=1 set together — switches are read once
per process, and no plain case is large enough for the product to take the wave form, so with the form barred every
case here runs as it does in the product; the one case that WOULD take the wave form at WAVE_MIN=1 shows the bar works),
"wave" (HIPSOXR_DEBUG_WAVE_MIN=1) or "nopair" (HIPSOXR_FFT_NO_PAIR).

Every job writes into a buffer filled with NaN (integers: a sentinel) with guards before and behind the result; every
result is checked against the oracle at the bars of tests/test_gpu_fft.py (float32 1e-6, float64 2e-9, float32 on float64
arithmetic 5e-8 relative RMS against the float64 direct form on the oracle's own bank; integer jobs: equal to the float
job of the same arithmetic width plus oracle.quantize, sample for sample, clip count included, as
tests/test_gpu_fft_pcm.py).  Prints one JSON line: per case the launch log's lines as text, the figures, digests of the results and what failed."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "python-soxr_amd"))
sys.path.insert(0, HERE)
import torch  # noqa: E402
import _table_probe as tp  # noqa: E402
import stream_fft_checks as sc  # noqa: E402
from soxr_amd import device as dev  # noqa: E402
from soxr_amd import dist as sdist  # noqa: E402
from oracle import oracle as o  # noqa: E402

AUTO, FFT, FFT_F64, FFT_PCM = dev._n.KERNEL_AUTO, dev._n.KERNEL_FFT, dev._n.KERNEL_FFT_F64, dev._n.KERNEL_FFT_PCM
PAD = 8
# child -> its switches (tests/test_gpu_fft_forms.py adds the debug-switch build and the launch log's path)
CHILDREN = {"plain": {"HIPSOXR_FFT_NO_WAVE": "1", "HIPSOXR_DEBUG_WAVE_MIN": "1"}, "wave": {"HIPSOXR_DEBUG_WAVE_MIN": "1"},
            "nopair": {"HIPSOXR_FFT_NO_PAIR": "1"}}
INT_SENT = {torch.int16: -12345, torch.int32: -123456789}
LOG = os.environ.get("HIPSOXR_DEBUG_LAUNCH_LOG", "")
_log_pos = 0
results = {}
_digests = []   # of every result of the running case: compared between two builds


def log_take():
    global _log_pos
    if not os.path.exists(LOG):
        return []
    with open(LOG) as f:
        f.seek(_log_pos)
        text = f.read()
        _log_pos = f.tell()
    return [l for l in text.splitlines() if l.strip()]


def note(y):
    _digests.append(hashlib.sha256(np.ascontiguousarray(y).tobytes()).hexdigest()[:16])
    return y


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(np.mean((a - b) ** 2)) / np.sqrt(np.mean(b ** 2))) if a.shape == b.shape and a.size else 9.0


def in_len_for(plan, n_out):
    """An input length whose output length is n_out (out_len is monotone in the input length)."""
    n = n_out * plan.M // plan.L
    while plan.out_len(n) < n_out:
        n += 1
    while plan.out_len(n) > n_out:
        n -= 1
    assert plan.out_len(n) == n_out
    return n


def guarded(n_out, ch, dtype):
    """-> (NaN- / sentinel-filled buffer of PAD + n_out + PAD frames, the view the job writes, the fill value)."""
    fill = INT_SENT.get(dtype, float("nan"))
    buf = torch.full((n_out + 2 * PAD,) if ch == 0 else (n_out + 2 * PAD, ch), fill, dtype=dtype, device="cuda")
    return buf, buf[PAD:PAD + n_out], fill


def untouched(t, fill):
    t = t.cpu().numpy()
    return bool(np.isnan(t).all()) if isinstance(fill, float) else bool((t == fill).all())


def run_job(plan, xt, kernel, fails, **kw):
    """One job through out= into a guarded buffer -> result (numpy) or None when it raised."""
    ch = 0 if xt.ndim == 1 else xt.shape[1]
    n_out = plan.out_len(xt.shape[0])
    buf, view, fill = guarded(n_out, ch, xt.dtype)
    try:
        dev.resample_tensor(plan, xt, out=view, kernel=kernel, **kw)
        torch.cuda.synchronize()
    except RuntimeError as e:
        fails.append(f"raised: {e}")
        return None
    if not (untouched(buf[:PAD], fill) and untouched(buf[PAD + n_out:], fill)):
        fails.append("a guard beside the result was overwritten")
    y = view.cpu().numpy()
    if (np.isnan(y).any() if isinstance(fill, float) else bool((y == fill).all())):
        fails.append("part of the result was not written")
    return note(y)


def case(name, one_round=False):
    def deco(fn):
        log_take()
        del _digests[:]
        fails, figs = [], {}
        print("FORMS_CASE", name, flush=True)
        fn(fails, figs)
        results[name] = dict(lines=log_take(), fails=fails, figs=figs, one_round=one_round, digests=list(_digests))
        return fn
    return deco


def float_case(fails, figs, plan, rates, quality, x, kernel, bar, **kw):
    y = run_job(plan, torch.from_numpy(x).cuda(), kernel, fails, **kw)
    if y is None:
        return
    ref = o.resample(x.astype(np.float64) if x.dtype == np.float64 or kernel == FFT_F64 else x, rates[0], rates[1], quality, mode="ref")
    figs["rel_rms"] = rel(y, ref)
    if not figs["rel_rms"] <= bar:
        fails.append(f"rel_rms {figs['rel_rms']:.3e} > {bar:.1e}")


def pcm_case(fails, figs, plan, x):
    """Integer job == float job of the same arithmetic width on the same values and layout + oracle.quantize."""
    xt = torch.from_numpy(x).cuda()
    counter = torch.zeros(1, dtype=torch.int64, device="cuda")
    y = run_job(plan, xt, FFT_PCM, fails, dither=True, dither_seed=7, clip_counter=counter)
    yf = run_job(plan, xt.float() if x.dtype == np.int16 else xt.double(), FFT, fails)
    if y is None or yf is None:
        return
    y2, yf2 = (y[:, None], yf[:, None]) if y.ndim == 1 else (y, yf)
    clips = 0
    for c in range(y2.shape[1]):
        want, n = o.quantize(np.ascontiguousarray(yf2[:, c]), x.dtype, channel=c, k0=0, dither=True, seed=7)
        clips += n
        nd = int(np.count_nonzero(want != y2[:, c]))
        figs[f"differ_ch{c}"] = nd
        if nd:
            fails.append(f"channel {c}: {nd} of {y2.shape[0]} samples differ from the float job + quantize")
    if int(counter.item()) != clips:
        fails.append(f"clip count {int(counter.item())}, host {clips}")


def stream_case(fails, figs, rates, ch, sizes, rng):
    """One TensorStream(engine="fft") fed `sizes` frames per call, every call into a guarded buffer of its own."""
    x = sc.signal(rng, sum(sizes), ch, np.float32)
    ts = dev.TensorStream(rates[0], rates[1], ch, dtype=torch.float32, quality="VHQ", engine="fft")
    fn, done = dev._n.lib.hipsoxr_stream_process_device, ts._done
    stream = torch.cuda.current_stream().cuda_stream
    xt = torch.from_numpy(x).cuda()
    outs, pos = [], 0
    row = max(ch, 1) * 4

    def call(ptr, n, cap):
        buf, view, fill = guarded(cap, 0 if ch == 1 else ch, torch.float32)
        dev._n.check(fn(ts._h, ptr, n, view.data_ptr(), cap, ts._done_ref, stream))
        torch.cuda.synchronize()
        got = done.value
        if not (untouched(buf[:PAD], fill) and untouched(buf[PAD + got:], fill)):
            fails.append("a stream call wrote outside the frames it reported")
        if np.isnan(view[:got].cpu().numpy()).any():
            fails.append("a stream call left reported frames unwritten")
        return note(view[:got].cpu().numpy())

    for i, n in enumerate(sizes):
        cap = int(n * ts._ratio) + ts._slack
        outs.append(call(xt.data_ptr() + pos * row, n, cap))
        pos += n
    while True:                                                  # the flush of last=True (TensorStream.resample_chunk)
        tail = call(None, 0, 4096)
        if tail.shape[0] == 0:
            break
        outs[-1] = np.concatenate([outs[-1], tail])
    ref = o.resample(x, rates[0], rates[1], "VHQ", mode="ref")
    taps = dev.Plan(rates[0], rates[1], "VHQ").taps
    try:
        figs["rel_rms"], figs["seam"] = sc.check_values(outs, ref, taps, 1e-6, "stream")
    except AssertionError as e:
        fails.append(f"stream values: {e}")


def raises_case(fails, plan, xt, kernel, text):
    try:
        dev.resample_tensor(plan, xt, kernel=kernel)
        torch.cuda.synchronize()
        fails.append("the job was served; a refusal was expected")
    except RuntimeError as e:
        if text not in str(e):
            fails.append(f"raised {e!r}, expected {text!r}")


def noise(rng, shape, dtype=np.float32):
    return (rng.standard_normal(shape) * 0.25).astype(dtype)


def main(child):
    rng = np.random.default_rng(2718)
    DOWN, UP, OFF = (48000, 44100), (44100, 48000), (48000, 40000)   # 147/160, 160/147 (both tabled), 5/6 (7-smooth, not tabled)
    down, up, off = (dev.Plan(*r, "VHQ") for r in (DOWN, UP, OFF))
    hop8 = tp.hop_out(down.L, down.M, down.taps, 8)                   # kept run of one quarter-size block (the row of small jobs)
    assert hop8 > 0
    n_pair1 = in_len_for(down, 2 * hop8 + 1)                          # one pair's kept run + 1 output: two work items
    wave_n = in_len_for(up, 2 * 3520 + 1)                             # k_fft_wave keeps 3520 outputs per block at 44.1k -> 48k

    if child == "plain":
        @case("mono_f32", one_round=True)
        def _(fails, figs):
            float_case(fails, figs, down, DOWN, "VHQ", noise(rng, n_pair1), FFT, 1e-6)

        @case("ragged_f32", one_round=True)
        def _(fails, figs):
            lens = [0, 1, 3000, 24 * down.M + 7]
            clips = [torch.from_numpy(noise(rng, n)).cuda() for n in lens]
            job = sdist.RaggedJob(down, clips, kernel=FFT)
            total = sum(job.n_out)
            buf, view, fill = guarded(total, 1, torch.float32)
            job._job.out, job.y = view.data_ptr(), view                # the same packed result, inside guards
            job.launch()
            torch.cuda.synchronize()
            if not (untouched(buf[:PAD], fill) and untouched(buf[PAD + total:], fill)):
                fails.append("a guard beside the packed result was overwritten")
            outs = [t.cpu().numpy().reshape(-1) for t in job.outputs()]
            note(view.cpu().numpy())
            if np.isnan(view.cpu().numpy()).any():
                fails.append("part of the packed result was not written")
            figs["rel_rms"] = max(rel(outs[i], o.resample(clips[i].cpu().numpy(), *DOWN, "VHQ", mode="ref")) for i in range(len(lens)) if lens[i])
            if outs[0].size or not figs["rel_rms"] <= 1e-6:
                fails.append(f"ragged: rel_rms {figs['rel_rms']:.3e}, empty clip gave {outs[0].size} frames")

        @case("il2_f32")
        def _(fails, figs):
            float_case(fails, figs, down, DOWN, "VHQ", noise(rng, (n_pair1, 2)), FFT, 1e-6)

        @case("il3_f32")
        def _(fails, figs):
            float_case(fails, figs, down, DOWN, "VHQ", noise(rng, (n_pair1, 3)), FFT, 1e-6)

        @case("mono_f64")
        def _(fails, figs):
            float_case(fails, figs, down, DOWN, "VHQ", noise(rng, n_pair1, np.float64), FFT, 2e-9)

        @case("mono_f32on64")
        def _(fails, figs):
            float_case(fails, figs, down, DOWN, "VHQ", noise(rng, n_pair1), FFT_F64, 5e-8)

        @case("mono_i16")
        def _(fails, figs):
            pcm_case(fails, figs, down, sc.signal(rng, n_pair1, 1, np.int16))

        @case("il2_i16")
        def _(fails, figs):
            pcm_case(fails, figs, down, sc.signal(rng, n_pair1, 2, np.int16))

        @case("mono_i32")
        def _(fails, figs):
            pcm_case(fails, figs, down, sc.signal(rng, n_pair1, 1, np.int32))

        @case("stream_mono_f32")
        def _(fails, figs):
            stream_case(fails, figs, DOWN, 1, [5000, 3001], rng)

        @case("stream_il2_f32")
        def _(fails, figs):
            stream_case(fails, figs, DOWN, 2, [5000, 3001], rng)

        @case("block_f32")
        def _(fails, figs):
            float_case(fails, figs, off, OFF, "VHQ", noise(rng, 12007), FFT, 1e-6)

        @case("none_f64_refused")
        def _(fails, figs):
            raises_case(fails, off, torch.from_numpy(noise(rng, 12007, np.float64)).cuda(), FFT, "FFT engine unavailable")

        @case("none_f64_auto")                                        # AUTO, >= 2^13 outputs: asked, declined, served by the exact engine
        def _(fails, figs):
            float_case(fails, figs, off, OFF, "VHQ", noise(rng, 12007, np.float64), AUTO, 2e-9)

        @case("two_stage_down_f32")                                   # inner launch_fft at 2:1 on the intermediate: in_abs0 = -pad
        def _(fails, figs):
            r = (48000, 44101.5)
            float_case(fails, figs, dev.Plan(*r, "VHQ"), r, "VHQ", noise(rng, 20011), AUTO, 1e-6)

        @case("wave_barred_f32", one_round=True)                      # the wave child's job: NO_WAVE bars what WAVE_MIN=1 would take
        def _(fails, figs):
            float_case(fails, figs, up, UP, "VHQ", noise(np.random.default_rng(31), wave_n), FFT, 1e-6)

    elif child == "wave":
        @case("wave_f32")
        def _(fails, figs):
            float_case(fails, figs, up, UP, "VHQ", noise(np.random.default_rng(31), wave_n), FFT, 1e-6)

    elif child == "nopair":
        @case("nopair_block_f32")
        def _(fails, figs):
            float_case(fails, figs, down, DOWN, "VHQ", noise(rng, n_pair1), FFT, 1e-6)

        @case("nopair_none_f64_refused")
        def _(fails, figs):
            raises_case(fails, down, torch.from_numpy(noise(rng, n_pair1, np.float64)).cuda(), FFT, "FFT engine unavailable")

        @case("nopair_none_f64_auto")
        def _(fails, figs):
            float_case(fails, figs, down, DOWN, "VHQ", noise(rng, 12007, np.float64), AUTO, 2e-9)
    else:
        raise SystemExit("child: plain | wave | nopair")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    print("FORMS_PROBE " + json.dumps(dict(cus=cus, cases=results)))


if __name__ == "__main__":
    main(sys.argv[1])
