"""GPU: equal-length jobs of the two-stage form (csrc/twostage.hip launch_two_stage) TRUNCATED below the plan's output length
(out_frames < out_len(in_frames)), down-sampling: the intermediate signal must reach as far past the job's last output as the
FFT stage's filter reads (poly_rules.h two_stage_mid_outputs) — sized by out_frames alone it ended where the signal goes on, and
the last outputs were the response to a signal cut short (2.5e-5 relative RMS on the last 3000 outputs of a clip truncated by 7).
Against the oracle's float64 direct form on windows of 3000 outputs at the head and the tail, with the bars of
tests/test_gpu_two_stage.py: relative RMS <= 1e-6 (float32) / 2e-9 (float64) of max(rms(ref), 0.05).  Truncated by 7 outputs
(inside the filter's reach: the intermediate ends with the signal) and by 1000 (beyond it: the intermediate ends a quarter of the
filter's taps past the job); one clip alone, mono and interleaved stereo, and a batch of three equal-length clips.  One spare frame
behind every clip keeps its sentinel.  An up-sampling job (its intermediate follows the input) rides along."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SENTINEL = 12345.0

CASES = [  # in rate, out rate, quality, dtype, bar, clips, channels, outputs cut
    (48000, 44101, "HQ", np.float32, 1e-6, 1, 1, 7),
    (48000, 44101, "HQ", np.float32, 1e-6, 1, 1, 1000),
    (48000, 44101, "VHQ", np.float64, 2e-9, 1, 1, 7),
    (44100, 16001, "HQ", np.float32, 1e-6, 1, 2, 7),
    (48000, 44101, "HQ", np.float32, 1e-6, 3, 1, 7),
    (44101, 48000, "HQ", np.float32, 1e-6, 1, 1, 7),
]


def _rms(v):
    return float(np.sqrt(np.mean(np.square(v, dtype=np.float64))))


@pytest.mark.parametrize("in_rate,out_rate,quality,dtype,tol,clips,ch,cut", CASES)
def test_truncated_job_matches_the_oracle_to_its_last_output(oracle, in_rate, out_rate, quality, dtype, tol, clips, ch, cut):
    import torch
    from soxr_amd import _native, device as dev
    plan = dev.Plan(in_rate, out_rate, quality)
    assert plan.phases > 0
    n = 30000
    n_out = plan.out_len(n) - cut
    assert min(n, n_out) >= 8192, "a job the two-stage form admits"
    rng = np.random.default_rng(cut + ch + clips)
    x = (rng.standard_normal((clips, n, ch)) * 0.25).astype(dtype)
    xt = torch.from_numpy(x).cuda()
    y = torch.full((clips, n_out + 1, ch), SENTINEL, dtype=xt.dtype, device="cuda")
    plan.run(xt.data_ptr(), y.data_ptr(), dev._torch_elem(xt.dtype), clips, ch, n, n_out, (n * ch, ch, 1), ((n_out + 1) * ch, ch, 1),
             stream=torch.cuda.current_stream().cuda_stream, kernel=_native.KERNEL_AUTO)
    ye = torch.empty((clips, n_out, ch), dtype=xt.dtype, device="cuda")
    plan.run(xt.data_ptr(), ye.data_ptr(), dev._torch_elem(xt.dtype), clips, ch, n, n_out, (n * ch, ch, 1), (n_out * ch, ch, 1),
             stream=torch.cuda.current_stream().cuda_stream, kernel=_native.KERNEL_EXACT)
    torch.cuda.synchronize()
    y, ye = y.cpu().numpy(), ye.cpu().numpy()
    assert np.all(y[:, n_out, :] == SENTINEL), "the frame behind a clip was written"
    assert not np.any(y[:, :n_out, :] == SENTINEL), "a payload element was not written"
    assert not np.array_equal(y[:, :n_out, :], ye), "AUTO did not take the two-stage form"
    pl = oracle.plan(in_rate, out_rate, quality)
    for c in range(clips):
        for k in range(ch):
            for k0 in (0, n_out - 3000):
                ref = oracle.resample_channel(pl, x[c, :, k].astype(np.float64), "ref", k0=k0, n_out=3000)
                err = _rms(y[c, k0:k0 + 3000, k].astype(np.float64) - ref) / max(_rms(ref), 0.05)
                assert err <= tol, "clip %d channel %d window at %d: %.3g" % (c, k, k0, err)
            # the very last outputs, where the intermediate used to end: absolute, at the scale of the signal
            ref = oracle.resample_channel(pl, x[c, :, k].astype(np.float64), "ref", k0=n_out - 64, n_out=64)
            assert np.max(np.abs(y[c, n_out - 64:n_out, k].astype(np.float64) - ref)) <= 8 * tol * 0.25
