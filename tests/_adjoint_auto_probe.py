"""Child process of tests/test_gpu_adjoint_auto.py, on the debug-switch build with a launch log: ragged adjoint jobs of
HIPSOXR_KERNEL_ADJOINT_AUTO on interpolated-phase plans, with the launch log's lines of each job.

    python _adjoint_auto_probe.py shape OUT.npz     the mixed table at 8 and at 40 clips, both directions, float32 — lines and the
                                                    8-clip values; then one two-stage clip per (tap count of k_poly_adj, width)
                                                    of _adjoint_two_stage_probe.COVER in ragged form, at the smallest admitted size
    python _adjoint_auto_probe.py budget OUT.npz    the 8-clip mixed tables again, HIPSOXR_DEBUG_POLY_MID_BUDGET set by the parent
                                                    (switches are read once per process): lines and values

(HIPSOXR_LIBRARY, HIPSOXR_DEBUG_LAUNCH_LOG set by the parent.)  After a HIP error the process ends: nothing further starts.
Also imported by the test for the mixed table and the C-level call."""
import os
import sys

import numpy as np

import _adjoint_two_stage_probe as tp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GUARD, POISON = 8, 12345.0
DIRECTIONS = {"down": (48000, 44101, "VHQ"), "up": (44101, 48000, "VHQ")}


def mixed_rows(plan):
    """(n_x, n_y, class) of the issue's mixed table, eight clips: the smallest admitted size, one more, one fewer (short), about
    20011, 4000 (short), a row without input, a clip without cotangent, a cotangent truncated by 1000."""
    n0 = tp.smallest(plan)
    big = 20011 if plan.out_len(20011) - 1000 >= tp.MIN_FRAMES and 20011 > n0 + 1 else n0 + int(1100 * plan.in_rate / plan.out_rate) + 1
    rows = [(n0, plan.out_len(n0), "two"), (n0 + 1, plan.out_len(n0 + 1), "two"), (n0 - 1, plan.out_len(n0 - 1), "short"),
            (big, plan.out_len(big), "two"), (4000, plan.out_len(4000), "short"), (0, 0, "empty"), (9000, 0, "zero"),
            (big + 500, plan.out_len(big + 500) - 1000, "two")]
    for n_x, n_y, cls in rows:  # the classes by the rule's own statement: 8192 frames or more either side
        assert (cls == "two") == (min(n_x, n_y) >= tp.MIN_FRAMES), (n_x, n_y, cls)
    return rows


class Job:
    """One ragged adjoint job on packed buffers: cotangents back to back, gradients GUARD poisoned frames apart."""

    def __init__(self, plan, rows, dtype, channels=1, seed=3):
        import torch
        self.plan, self.rows, self.ch = plan, rows, channels
        gen = torch.Generator(device="cuda").manual_seed(seed)
        self.gy = torch.randn(max(1, sum(r[1] for r in rows)), channels, dtype=dtype, device="cuda", generator=gen)
        self.gx = torch.full((sum(r[0] + GUARD for r in rows) + GUARD, channels), POISON, dtype=dtype, device="cuda")
        table, py, px = [], 0, GUARD
        for n_x, n_y, _ in rows:
            table.append([py * channels, n_y, px * channels, n_x])
            py += n_y
            px += n_x + GUARD
        self.table = np.asarray(table, np.int64).reshape(-1, 4)

    def run(self, kernel):
        import torch
        from soxr_amd import device as dev
        self.plan.run_adjoint_ragged(self.gy.data_ptr(), self.gx.data_ptr(), dev._torch_elem(self.gy.dtype), self.ch, self.table, (self.ch, 1), (self.ch, 1),
                                     stream=torch.cuda.current_stream().cuda_stream, kernel=kernel)
        return self.gx

    def clip_gy(self, c):
        off, n_y = int(self.table[c, 0]) // self.ch, int(self.table[c, 1])
        return self.gy[off:off + n_y]

    def clip_gx(self, c):
        off, n_x = int(self.table[c, 2]) // self.ch, int(self.table[c, 3])
        return self.gx[off:off + n_x]

    def guards(self):
        """every element of gx outside the clips"""
        import torch
        mask = torch.ones(self.gx.shape[0], dtype=torch.bool, device="cuda")
        for c in range(len(self.rows)):
            off, n_x = int(self.table[c, 2]) // self.ch, int(self.table[c, 3])
            mask[off:off + n_x] = False
        return self.gx[mask]


def fields(line):
    return dict(tok.split("=", 1) for tok in line.split() if "=" in tok)


def _logged(log_path, fn):
    import torch
    torch.cuda.synchronize()
    open(log_path, "w").close()
    r = fn()
    torch.cuda.synchronize()
    with open(log_path) as f:
        return r, f.read()


def main(mode, out_path):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "python-soxr_amd")]
    import torch
    from soxr_amd import device as dev
    log_path = os.environ["HIPSOXR_DEBUG_LAUNCH_LOG"]
    K = dev.KERNEL_ADJOINT_AUTO
    out = {}
    for name, case in sorted(DIRECTIONS.items()):
        plan = dev.Plan(*case)
        for reps in (1, 5) if mode == "shape" else (1,):
            job = Job(plan, mixed_rows(plan) * reps, torch.float32)
            job.run(K)  # (tables and pools: the logged run is the second)
            gx, log = _logged(log_path, lambda: job.run(K))
            out["log_%s_%d" % (name, 8 * reps)] = log
            if reps == 1:
                out["gx_%s" % name] = gx.cpu().numpy()
    if mode == "shape":
        for taps, case in sorted(tp.COVER.items()):
            plan = dev.Plan(*case)
            assert plan.phases and tp.poly_taps(plan) == taps, (case, taps)
            n_x = tp.smallest(plan)
            for kind, dt in (("f32", torch.float32), ("f64", torch.float64)):
                if kind == "f64" and taps > tp.F64_MAX_TAPS:
                    continue
                job = Job(plan, [(n_x, plan.out_len(n_x), "two")], dt, seed=taps)
                ref = dev.resample_tensor_adjoint(plan, job.clip_gy(0)[:, 0].double(), n_x, kernel=dev.KERNEL_ADJOINT)
                _, log = _logged(log_path, lambda: job.run(K))
                out["log_%d_%s" % (taps, kind)] = log
                out["got_%d_%s" % (taps, kind)] = job.clip_gx(0)[:, 0].cpu().numpy()
                out["ref_%d_%s" % (taps, kind)] = ref.cpu().numpy()
                out["guards_%d_%s" % (taps, kind)] = bool((job.guards() == POISON).all())
    np.savez(out_path, **out)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
