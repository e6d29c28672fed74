"""Device-resident, batched entry points — what the reference cannot express (it has no GPU and no
batch axis; its only "batch" is the channel axis, src/soxr/__init__.py:22).

`Plan` owns the shared filter bank (what soxr_create designs per handle).  `resample_tensor`
runs the hot path on torch tensors that already live in HBM, with no host round trip; this is the
path bench.py times.  torch is used only for device memory and streams.
"""
import ctypes as _C

import numpy as np

from . import _native as _n
from . import _quality_to_enum
from ._job import make_job as _make_job, table_job as _table_job, refusal as _refusal
from ._native import (KERNEL_AUTO, KERNEL_GATHER, KERNEL_TILE, KERNEL_TILE_VALU, KERNEL_TILE_MFMA,  # noqa: F401
                      KERNEL_FFT, KERNEL_EXACT, KERNEL_WAVE_DOT, KERNEL_FFT_F64, KERNEL_FFT_PCM, KERNEL_ADJOINT,
                      KERNEL_ADJOINT_FFT, KERNEL_ADJOINT_TWO_STAGE, KERNEL_ADJOINT_AUTO)


class Plan:
    """Immutable conversion plan: ratio L/M, polyphase bank, device tables (built lazily)."""

    def __init__(self, in_rate, out_rate, quality="HQ", vr=False):
        """vr=True: the plan of a variable-rate stream (always an interpolated-phase table)."""
        if in_rate <= 0 or out_rate <= 0:
            raise ValueError("Sample rate should be over 0")
        self._h = _C.c_void_p()
        create = _n.lib.hipsoxr_plan_create_vr if vr else _n.lib.hipsoxr_plan_create
        _n.check(create(float(in_rate), float(out_rate), _quality_to_enum(quality), _C.byref(self._h)))
        info = _n.PlanInfo()
        _n.check(_n.lib.hipsoxr_plan_info(self._h, _C.byref(info)))
        self.in_rate, self.out_rate = info.in_rate, info.out_rate
        self.L, self.M, self.taps = int(info.L), int(info.M), int(info.taps)
        self.phases = int(info.interpolated)  # 0: exact bank; P: interpolated-phase plan
        self.precision_bits, self.passband_end = info.precision_bits, info.passband_end
        self.stopband_begin, self.att_db, self.kaiser_beta = info.stopband_begin, info.att_db, info.kaiser_beta
        self.vr = bool(vr)  # a variable-rate plan: in_rate / out_rate is the largest io ratio (`run_vr_ragged`, dist.resample_varispeed)

    def __del__(self, _delete=_n.lib.hipsoxr_plan_delete):  # bound early: module globals may be gone at exit
        h = getattr(self, "_h", None)
        if h:
            _delete(h)
            self._h = None

    @property
    def handle(self):
        return self._h

    def out_len(self, n_in):
        return int(_n.lib.hipsoxr_plan_out_len(self._h, int(n_in)))

    def vr_out_len(self, n_in, io_ratio):
        """Frames a variable-rate stream of this plan emits in all for n_in input frames at the constant io ratio `io_ratio`
        (input frames per output frame; hipsoxr_plan_vr_out_len).  0 on a plan that is not `vr`, and for a ratio the plan
        does not admit (above in_rate / out_rate, or outside (2^-20, 2^20))."""
        return int(_n.lib.hipsoxr_plan_vr_out_len(self._h, int(n_in), float(io_ratio)))

    def bank(self):
        """float64 bank: phase-major [L][taps], or the cubic table [P][taps][4] of an
        interpolated-phase plan."""
        shape = (self.phases, self.taps, 4) if self.phases else (self.L, self.taps)
        b = np.empty(shape, np.float64)
        _n.check(_n.lib.hipsoxr_plan_get_bank(self._h, b.ctypes.data, b.size))
        return b

    def set_bank(self, bank):
        """Install a bank (e.g. the one broadcast from rank 0 over RCCL); device tables rebuild."""
        b = np.ascontiguousarray(bank, np.float64)
        _n.check(_n.lib.hipsoxr_plan_set_bank(self._h, b.ctypes.data, b.size))

    def run(self, in_ptr, out_ptr, elem, n_clips, n_channels, in_frames, out_frames, in_strides,
            out_strides, stream=None, kernel=_n.KERNEL_AUTO, in_abs0=0, out_k0=0, clip_counter=None,
            dither=False, dither_seed=0):
        """Raw launch: device pointers (ints), strides = (clip, frame, channel) in elements."""
        j = _make_job(in_ptr, out_ptr, elem, kernel, n_clips, n_channels, in_strides, out_strides, in_frames, out_frames,
                      in_abs0, out_k0, clip_counter, dither, dither_seed)
        err = _n.lib.hipsoxr_run_device(self._h, j, stream)  # (ctypes passes the struct by reference: argtypes says POINTER(Job))
        if err:
            _n.check(err)

    def run_adjoint(self, gy_ptr, gx_ptr, elem, n_clips, n_channels, gy_frames, gx_frames, gy_strides, gx_strides,
                    stream=None, kernel=_n.KERNEL_AUTO, clip_table=None):
        """Raw launch of the transposed operator (hipsoxr_run_device_adjoint): gx = A^T gy for the forward job A that
        `run(..., kernel=KERNEL_EXACT)` computes — gy has gy_frames <= out_len(gx_frames) frames, gx has gx_frames.
        Device pointers (ints), strides = (clip, frame, channel) in elements.  float32 / float64, exact-bank plans;
        kernel=KERNEL_ADJOINT: every constant-rate plan, interpolated-phase plans included."""
        j = _make_job(gy_ptr, gx_ptr, elem, kernel, n_clips, n_channels, gy_strides, gx_strides, gy_frames, gx_frames,
                      clip_table=clip_table)
        _n.check(_n.lib.hipsoxr_run_device_adjoint(self._h, _C.byref(j), stream))

    def run_adjoint_ragged(self, gy_ptr, gx_ptr, elem, n_channels, table, gy_strides, gx_strides, stream=None,
                           kernel=_n.KERNEL_AUTO, table_dev=None):
        """Raw launch of the transposed operator over a ragged batch (hipsoxr_run_device_adjoint_ragged): ONE launch for
        all clips.  table: int64 host array [n_clips, 4] of rows (gy offset, n_y, gx offset, n_x), offsets in elements
        from gy_ptr / gx_ptr, n_y <= out_len(n_x) per clip; table_dev: a device copy of it (pointer), or None = uploaded
        in stream order.  strides = (frame, channel) in elements.  Selectors as for `run_adjoint`."""
        t, n, n_y, n_x, _ = _table_job(table)
        j = _make_job(gy_ptr, gx_ptr, elem, kernel, n, n_channels, gy_strides, gx_strides, n_y, n_x,
                      clip_table=t.ctypes.data, clip_table_dev=table_dev)
        _n.check(_n.lib.hipsoxr_run_device_adjoint_ragged(self._h, _C.byref(j), stream))

    def run_vr_ragged(self, in_ptr, out_ptr, elem, n_channels, table, io_ratios, in_strides, out_strides, stream=None,
                      kernel=_n.KERNEL_AUTO, table_dev=None, clip_counter=None, dither=False, dither_seed=0):
        """Raw launch of a ragged batch with a rate per clip (hipsoxr_run_device_vr_ragged) on a `vr` plan: ONE launch for
        all clips, clip c resampled at io_ratios[c] (input frames per output frame, at most in_rate / out_rate).  table:
        int64 host array [n_clips, 4] of rows (in offset, n_in, out offset, n_out), offsets in elements from in_ptr /
        out_ptr, n_out <= vr_out_len(n_in, io_ratios[c]) per clip; table_dev: a device copy of it (pointer), or None =
        uploaded in stream order.  strides = (frame, channel) in elements.  KERNEL_AUTO, KERNEL_EXACT and KERNEL_GATHER
        all run the exact engine: each clip has the bits of a variable-rate stream set to its ratio and fed the clip."""
        t, n, n_in, n_out, r = _table_job(table, io_ratios)
        j = _make_job(in_ptr, out_ptr, elem, kernel, n, n_channels, in_strides, out_strides, n_in, n_out,
                      clip_counter=clip_counter, dither=dither, dither_seed=dither_seed,
                      clip_table=t.ctypes.data, clip_table_dev=table_dev)
        _n.check(_n.lib.hipsoxr_run_device_vr_ragged(self._h, _C.byref(j), r.ctypes.data, stream))

    def run_vr_ragged_adjoint(self, gy_ptr, gx_ptr, elem, n_channels, table, io_ratios, gy_strides, gx_strides, stream=None,
                              kernel=_n.KERNEL_AUTO, table_dev=None):
        """Raw launch of the transposed operator of `run_vr_ragged` (hipsoxr_run_device_vr_ragged_adjoint) on a `vr` plan:
        ONE launch for all clips, gx[c] = A_c^T gy[c] with A_c the forward of n_x[c] input frames at io_ratios[c].  table:
        int64 host array [n_clips, 4] of rows (gy offset, n_y, gx offset, n_x), offsets in elements from gy_ptr / gx_ptr,
        n_y <= vr_out_len(n_x, io_ratios[c]) per clip; table_dev: a device copy of it (pointer), or None = uploaded in
        stream order.  strides = (frame, channel) in elements.  float32 / float64; KERNEL_AUTO and KERNEL_ADJOINT run
        the same launch."""
        t, n, n_y, n_x, r = _table_job(table, io_ratios)
        j = _make_job(gy_ptr, gx_ptr, elem, kernel, n, n_channels, gy_strides, gx_strides, n_y, n_x,
                      clip_table=t.ctypes.data, clip_table_dev=table_dev)
        _n.check(_n.lib.hipsoxr_run_device_vr_ragged_adjoint(self._h, _C.byref(j), r.ctypes.data, stream))


class PreparedJob:
    """A device job whose descriptor is built once: `launch()` is a single C call
    (hipsoxr_run_device).  For loops that re-run the same conversion on the same buffers
    (benchmarks, fixed-shape pipelines) where Python-side argument handling would otherwise
    cost as much as the 13 us kernel."""

    def __init__(self, plan, x, out, kernel=_n.KERNEL_AUTO, dither=False, clip_counter=None, dither_seed=0):
        import torch
        x3, o3 = _as3(x), _as3(out)
        clips, frames, ch = x3.shape
        if tuple(o3.shape) != (clips, plan.out_len(frames), ch):
            raise ValueError("out has the wrong shape for this plan")
        j = _make_job(x3.data_ptr(), o3.data_ptr(), _torch_elem(x.dtype), kernel, clips, ch, x3.stride(), o3.stride(),
                      frames, o3.shape[1], clip_counter=clip_counter.data_ptr() if clip_counter is not None else None,
                      dither=dither, dither_seed=dither_seed)
        self._job, self._ref = j, _C.byref(j)
        self._plan, self._keep = plan, (x, out, clip_counter)
        self._stream = torch.cuda.current_stream(x.device).cuda_stream
        self._fn, self._h = _n.lib.hipsoxr_run_device, plan.handle

    def launch(self):
        err = self._fn(self._h, self._ref, self._stream)
        if err:
            _n.check(err)


_TORCH_ELEM = None


def _torch_elem(dtype):
    """Element type of a device JOB (resample_tensor, PreparedJob, RaggedJob, the adjoint): the four stream types and
    float16 / bfloat16."""
    global _TORCH_ELEM
    import torch
    if _TORCH_ELEM is None:
        _TORCH_ELEM = {torch.float32: _n.F32, torch.float64: _n.F64, torch.int32: _n.I32,
                       torch.int16: _n.I16, torch.float16: _n.F16, torch.bfloat16: _n.BF16}
    try:
        return _TORCH_ELEM[dtype]
    except KeyError:
        raise TypeError(f"Data type must be one of [float32, float64, int16, int32, float16, bfloat16], not {dtype}")


def _torch_stream_elem(dtype):
    """Element type of a STREAM (TensorStream, TensorStreamGroup): the io types libsoxr's streams have — no half types."""
    elem = _torch_elem(dtype)
    if elem in (_n.F16, _n.BF16):
        raise TypeError("Data type must be one of [float32, float64, int16, int32, float16, bfloat16] for device jobs; "
                        f"streams take four of them, [float32, float64, int16, int32], not {dtype}")
    return elem


def _as3(t):
    if t.ndim == 1:
        return t[None, :, None]
    if t.ndim == 2:
        return t[None]
    if t.ndim != 3:
        raise ValueError("Input must be 1-D, 2-D or 3-D")
    return t


def _like_rank(t3, ndim):
    return t3[0, :, 0] if ndim == 1 else (t3[0] if ndim == 2 else t3)


def _adjoint_refusal(plan, elem, kernel=_n.KERNEL_AUTO):
    """The C entry's own refusal of (plan, element type, selector) for an adjoint job, or None: asked with an empty job, so
    that a forward that could not be differentiated fails when it is called, not in the middle of backward."""
    return _refusal(plan.run_adjoint, None, None, elem, 0, 0, 0, 0, (0, 0, 0), (0, 0, 0), kernel=kernel)


def _adjoint_forward_kernel(kernel):
    """The forward selector an adjoint's own backward runs: the engine the adjoint ran on — KERNEL_FFT for
    KERNEL_ADJOINT_FFT, KERNEL_AUTO (the two-stage form on the plans that selector serves) for KERNEL_ADJOINT_TWO_STAGE,
    KERNEL_AUTO for KERNEL_ADJOINT_AUTO (which is defined as the transpose of that selector's forward), the exact engine
    for every other selector."""
    if kernel in (_n.KERNEL_ADJOINT_TWO_STAGE, _n.KERNEL_ADJOINT_AUTO):
        return _n.KERNEL_AUTO
    return _n.KERNEL_FFT if kernel == _n.KERNEL_ADJOINT_FFT else _n.KERNEL_EXACT


def resample_tensor_adjoint(plan, gy, in_frames, out=None, kernel=_n.KERNEL_AUTO):
    """The transposed operator as a function: gx = A^T gy, where A is the resample of `in_frames` input frames that
    `resample_tensor(plan, x, kernel=KERNEL_EXACT)` computes (what its backward pass runs; the adjoint an iterative
    solver needs).  On the current torch stream, asynchronously.

    gy : [frames] | [frames, channels] | [clips, frames, channels] float32 / float64 device tensor, any strides, with at
         most plan.out_len(in_frames) frames (a truncated forward output has a truncated cotangent).
    Returns a tensor of the same rank with in_frames frames (`out` may be supplied); every element is written.
    Gather form on the transposed bank, no atomics: bitwise reproducible, independent of layout.  Differentiable (its
    backward is the forward on the exact engine).  kernel=KERNEL_AUTO / KERNEL_EXACT: exact-bank plans only (an
    interpolated-phase plan is refused by name).  kernel=KERNEL_ADJOINT: every constant-rate plan — on an exact-bank plan
    the same launch and the same bits, on an interpolated-phase plan (`plan.phases != 0`: 48000 -> 44101, non-integral
    rates) the gather-form adjoint on the plan's interpolation table, whose coefficients are the very bits the forward
    with kernel=KERNEL_EXACT multiplies by.  There a non-finite gy[k] reaches exactly the frames of its true support.
    Ragged batches: `dist.resample_ragged_adjoint` / `dist.resample_ragged`.  The two-stage form's adjoint, variable
    rate, streams and integer types are not served.  float16 / bfloat16 cotangents: the float32 adjoint on `gy.float()`,
    rounded once (every selector above; not the ragged entry).

    kernel=KERNEL_ADJOINT_FFT: the adjoint on the frequency-domain engine, for exact-bank HQ / VHQ plans — the forward
    float job of the plan's transposed plan (L' = M, M' = L, the mirrored prototype: the same coefficients) on the kernels
    KERNEL_FFT runs, at about that engine's cost for the reversed ratio.  1e-6-class (float32; float64: 2e-9 VHQ, 1e-6
    HQ), not bit-identical to the exact adjoint; opt-in by name, the defaults keep their bits.  Its own backward is the
    forward with KERNEL_FFT.  Interpolated-phase and variable-rate plans, recipes below HQ and integer types are refused
    by name, and a plan or layout the engine has no form for raises ("unavailable") — it never runs the exact adjoint.

    kernel=KERNEL_ADJOINT_TWO_STAGE: the transposed two-stage form, for the interpolated-phase HQ / VHQ plans (arbitrary
    ratios) whose float forward KERNEL_AUTO runs on that form — the transpose of that very job, stage by stage: the FFT
    stage's transposed plan on the frequency-domain engine and `k_poly_adj`, the gather-form transpose of the polyphase
    stage on the forward's own table and positions (no atomics: bitwise reproducible).  About the forward form's cost where
    KERNEL_ADJOINT walks the plan's full tap count; in the form's class against the exact adjoint, 1e-6 (float32) / 2e-9
    VHQ, 1e-6 HQ (float64).  Its own backward is the forward under KERNEL_AUTO.  float32 / float64 (float16 / bfloat16
    widened), any clips x channels and strides.  Exact-bank and variable-rate plans, integer types and clip tables
    (`dist.resample_ragged*`) are refused by name; a plan without the form, fewer than 8192 frames either side or an FFT
    stage that declines raises ("unavailable", naming KERNEL_ADJOINT) — it never runs the exact adjoint.

    kernel=KERNEL_ADJOINT_AUTO: the transpose of the job `resample_tensor(plan, x)` launches under KERNEL_AUTO for the same
    plan and shape — the selector that picks the fast adjoint where there is one and never raises "unavailable".  It
    resolves to KERNEL_ADJOINT_FFT's launch on an exact-bank HQ / VHQ plan from 8192 cotangent elements in all (frames x
    clips x channels, the forward's own threshold), to KERNEL_ADJOINT_TWO_STAGE's launch on an interpolated-phase plan
    with the form and 8192 frames either side, and to KERNEL_ADJOINT's exact adjoint everywhere else (short jobs, recipes
    below HQ, an engine that declines, HIPSOXR_NO_FFT / HIPSOXR_NO_TWO_STAGE) — with that selector's bits in each case.
    Its own backward is the forward under KERNEL_AUTO.  Refused by name: what KERNEL_ADJOINT refuses (integer types,
    variable-rate plans, clip tables on this entry).  KERNEL_AUTO / KERNEL_EXACT here keep their meaning and their bits."""
    if not gy.is_cuda:
        raise RuntimeError("resample_tensor needs a device tensor (soxr_amd has no CPU fallback)")
    import torch
    if out is None and gy.requires_grad and torch.is_grad_enabled():
        return _autograd_fns()[1].apply(gy, plan, int(in_frames), kernel)
    if out is not None and gy.requires_grad and torch.is_grad_enabled():
        raise ValueError("out= cannot be combined with a tensor that requires grad")
    return _adjoint_plain(plan, gy, int(in_frames), out, kernel)


def _adjoint_plain(plan, gy, in_frames, out=None, kernel=_n.KERNEL_AUTO):
    import torch
    elem = _torch_elem(gy.dtype)
    g3 = _as3(gy)
    clips, n_y, ch = g3.shape
    if out is None:
        o3 = torch.empty((clips, in_frames, ch), dtype=gy.dtype, device=gy.device)
    else:
        o3 = _as3(out)
        if tuple(o3.shape) != (clips, in_frames, ch) or out.dtype != gy.dtype:
            raise ValueError(f"out has shape {tuple(out.shape)}, expected frames={in_frames}")
    stream = torch.cuda.current_stream(gy.device).cuda_stream
    # (an empty job still goes to the C entry: it is what refuses an integer type or an interpolated-phase plan)
    plan.run_adjoint(g3.data_ptr(), o3.data_ptr(), elem, clips, ch, n_y, in_frames, tuple(g3.stride()),
                     tuple(o3.stride()), stream=stream, kernel=kernel)
    return _like_rank(o3, gy.ndim)


_AUTOGRAD = None


def _autograd_fns():
    """The torch.autograd.Function pair (built on first use: torch is imported lazily everywhere in this module).
    Resampling is linear: the forward's backward is the adjoint, the adjoint's backward is the forward on the exact
    engine — so double backward works and both functions are differentiable to any order."""
    global _AUTOGRAD
    if _AUTOGRAD is not None:
        return _AUTOGRAD
    import torch

    class ResampleFn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, plan, kernel, grad_kernel):
            ctx.plan, ctx.frames, ctx.grad_kernel = plan, _as3(x).shape[1], grad_kernel
            return _resample_plain(plan, x.detach(), kernel=kernel)

        @staticmethod
        def backward(ctx, gy):
            return resample_tensor_adjoint(ctx.plan, gy, ctx.frames, kernel=ctx.grad_kernel), None, None, None

    class AdjointFn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, gy, plan, in_frames, kernel):
            ctx.plan, ctx.n_y, ctx.kernel = plan, _as3(gy).shape[1], kernel
            return _adjoint_plain(plan, gy.detach(), in_frames, kernel=kernel)

        @staticmethod
        def backward(ctx, ggx):  # (the forward on the exact engine; its own gradient is this adjoint again, same selector)
            y = resample_tensor(ctx.plan, ggx, kernel=_adjoint_forward_kernel(ctx.kernel), grad_kernel=ctx.kernel)
            return y.narrow(y.ndim - 2 if y.ndim > 1 else 0, 0, ctx.n_y), None, None, None

    _AUTOGRAD = (ResampleFn, AdjointFn)
    return _AUTOGRAD


def resample_tensor(plan, x, out=None, kernel=_n.KERNEL_AUTO, dither=False, clip_counter=None, dither_seed=0,
                    grad_kernel=_n.KERNEL_AUTO):
    """Resample a device tensor on the current torch stream, asynchronously.

    x : [frames] | [frames, channels] | [clips, frames, channels] torch tensor on a HIP device
        (any strides; channel-last is the python-soxr [frame, channel] convention).
    Returns a tensor of the same rank with plan.out_len(frames) frames (`out` may be supplied).
    Integer tensors: dither / dither_seed = TPDF dither on int16 output, keyed by (seed, channel, output index);
    clip_counter = a one-element int64 / uint64 device tensor that counts saturated outputs.  AUTO keeps them on the
    canonical-order engine; kernel=KERNEL_FFT_PCM asks for the frequency-domain engine (int16 in float32, int32 in
    float64 arithmetic, the same output stage: within 1 LSB of the canonical order, not bit-identical to it).
    float16 / bfloat16 tensors: the result has the input's type and is, bit for bit, the float32 job of the same `kernel`
    on `x.float()` rounded once to nearest even (`.to(x.dtype)`: NaN, +-inf, overflow to +-inf and float16 subnormals
    included) — fused into the frequency-domain engine's kernels for unit-stride columns and interleaved channel pairs of the
    tabled ratios (by name, or AUTO from 2^13 outputs in all), a widening and a narrowing pass around the float32 job
    otherwise.  KERNEL_FFT_PCM, KERNEL_FFT_F64 and KERNEL_WAVE_DOT refuse them; dither / clip_counter are ignored.

    Differentiable: when x.requires_grad (and grad mode is on) the result carries a grad_fn whose backward is the
    transposed operator (`resample_tensor_adjoint`), so gradients — and gradients of gradients — flow through a
    resample.  `kernel` is honoured for the forward; `out=` is then a ValueError; plans the adjoint does not serve
    (interpolated-phase plans, integer tensors) raise when the forward is called.  The gradient is the EXACT engine's
    adjoint: where AUTO sends a large forward to the frequency-domain engine, forward and gradient agree in that engine's
    1e-6 class, not to rounding (kernel=KERNEL_EXACT: to rounding).  Without requires_grad nothing changes.

    grad_kernel is the selector the backward's adjoint runs with.  The default refuses an interpolated-phase plan
    (`plan.phases != 0`) as before; grad_kernel=KERNEL_ADJOINT admits it — the check is still made when the forward is
    called — and the gradient is then the adjoint of the forward the exact engine computes on that plan.  Under
    kernel=KERNEL_AUTO a float job of an interpolated-phase plan runs the two-stage form, so forward and gradient agree in
    that form's class, 1e-6 (float32) / 2e-9 (float64); with kernel=KERNEL_EXACT they agree to rounding.
    grad_kernel=KERNEL_ADJOINT_FFT (exact-bank HQ / VHQ plans): the backward runs on the frequency-domain engine, at about
    the forward's own cost there instead of several times it — see `resample_tensor_adjoint`; forward and gradient agree
    in that engine's class.  What it refuses is raised when the forward is called, as for the other selectors.
    grad_kernel=KERNEL_ADJOINT_TWO_STAGE (interpolated-phase HQ / VHQ plans): the backward is the transpose of the two-stage
    form that kernel=KERNEL_AUTO runs on such a plan, at about that form's cost — forward and gradient then transpose each
    other to rounding, not only in the 1e-6 class.  Jobs the form does not admit (fewer than 8192 frames either side)
    raise in backward ("unavailable"); no fast gradient is ever chosen by AUTO.
    grad_kernel=KERNEL_ADJOINT_AUTO: the backward is the transpose of whatever kernel=KERNEL_AUTO launches for the plan and
    shape — KERNEL_ADJOINT_FFT's launch, KERNEL_ADJOINT_TWO_STAGE's, or the exact adjoint where no fast form takes the
    job (see `resample_tensor_adjoint`); it never raises "unavailable", so one value serves every plan and length.
    """
    if x.is_cuda and x.requires_grad:
        import torch
        if torch.is_grad_enabled():
            if out is not None:
                raise ValueError("out= cannot be combined with a tensor that requires grad")
            why = _adjoint_refusal(plan, _torch_elem(x.dtype), grad_kernel)
            if why:
                raise RuntimeError(why)
            return _autograd_fns()[0].apply(x, plan, kernel, grad_kernel)
    return _resample_plain(plan, x, out, kernel, dither, clip_counter, dither_seed)


def _resample_plain(plan, x, out=None, kernel=_n.KERNEL_AUTO, dither=False, clip_counter=None, dither_seed=0):
    """`resample_tensor` proper: the launch, without autograd."""
    import torch
    if not x.is_cuda:
        raise RuntimeError("resample_tensor needs a device tensor (soxr_amd has no CPU fallback)")
    elem = _torch_elem(x.dtype)
    x3 = _as3(x)
    clips, frames, ch = x3.shape
    n_out = plan.out_len(frames)
    if out is None:
        o3 = torch.empty((clips, n_out, ch), dtype=x.dtype, device=x.device)
    else:
        o3 = _as3(out)
        if tuple(o3.shape) != (clips, n_out, ch):
            raise ValueError(f"out has shape {tuple(out.shape)}, expected frames={n_out}")
    cc = clip_counter.data_ptr() if clip_counter is not None else None
    if n_out and clips and ch:
        stream = torch.cuda.current_stream(x.device).cuda_stream
        plan.run(x3.data_ptr(), o3.data_ptr(), elem, clips, ch, frames, n_out, tuple(x3.stride()),
                 tuple(o3.stride()), stream=stream, kernel=kernel, clip_counter=cc, dither=dither, dither_seed=dither_seed)
    return _like_rank(o3, x.ndim)


class TensorStream:
    """Device-resident counterpart of `ResampleStream` (reference: src/soxr/__init__.py:56-131, CSoxr::process
    src/soxr_ext.cpp:129-187): chunks are torch tensors that already live in HBM, the pending input stays there, and a
    call enqueues one device-to-device copy and one launch on the current torch stream — no copy over PCIe, no host
    synchronisation (`hipsoxr_stream_process_device`: the stream handle's counters, ring and clock, device pointers).

        ts = TensorStream(44100, 16000, num_channels=2, dtype=torch.int16, quality="VHQ")
        y = ts.resample_chunk(x_dev)            # x_dev: [frames] (mono) or [frames, channels]
        tail = ts.resample_chunk(x_last, last=True)

    The same frames come out of the same calls as from `ResampleStream` on the same input, and the concatenated output
    is the one-shot result bit for bit (canonical-order engine: every output is a pure function of absolute positions)
    — the property the reference's test_stream_length / test_divide_match pin for its own streams.  vr=True: a
    variable-rate stream (`set_io_ratio`), in_rate / out_rate the LARGEST io ratio that will be used.  int16 output is
    dithered as the host stream's is (dither=False: off).  Like every torch op a call is ordered on the CURRENT
    stream: use one torch stream per TensorStream, or synchronise.

    engine="fft" (HIPSOXR_STREAM_FFT, opt-in): every call emits the same number of frames as the default stream — same
    delay(), same flush — but computes them on the frequency-domain engine: 1e-6-class values (integers within 1 LSB of
    the default), NOT bit-identical to the default stream or to another cut of the signal into chunks.  For callers who
    feed seconds of audio per call: measured 1.3-1.9x faster per call at 0.1-1 s chunks, 1.5-3x at 10 s, 2.2-4x at 60 s
    (48k -> 44.1k mono / stereo, 44.1k -> 16k 8 channels, VHQ; ahead from the shortest chunk measured, 0.1 s — no
    crossover inside the measured range, profiles/NOTES_stream_fft.md).  HQ / VHQ on the engine's tabled ratios, constant
    rate; float32 / float64 any channel count, int16 mono or even channel counts, int32 mono — anything else raises at
    creation with the reason."""

    def __init__(self, in_rate, out_rate, num_channels=1, dtype=None, quality="HQ", vr=False, dither=True, dither_seed=0,
                 engine="exact"):
        import torch
        if in_rate <= 0 or out_rate <= 0:
            raise ValueError("Sample rate should be over 0")
        if num_channels < 1 or num_channels > 65536:
            raise ValueError("Invalid number of channels")
        if engine not in ("exact", "fft"):
            raise ValueError("engine must be 'exact' or 'fft'")
        self.engine = engine
        self.channels = int(num_channels)
        self.dtype = torch.float32 if dtype is None else dtype
        self._elem = _torch_stream_elem(self.dtype)
        self._ratio = float(out_rate) / float(in_rate)
        self._h = _C.c_void_p()
        flags = (_n.VR if vr else 0) | (0 if dither else _n.NO_DITHER) | (_n.STREAM_FFT if engine == "fft" else 0)
        _n.check(_n.lib.hipsoxr_stream_create(float(in_rate), float(out_rate), self.channels, self._elem,
                                              _quality_to_enum(quality), flags, _C.byref(self._h)))
        if dither_seed:
            _n.check(_n.lib.hipsoxr_stream_set_dither_seed(self._h, int(dither_seed) & 0xFFFFFFFF))
        self._vr = bool(vr)
        self._done = _C.c_size_t(0)
        self._done_ref = _C.byref(self._done)
        self._ended = False
        info = _n.PlanInfo()
        _n.check(_n.lib.hipsoxr_plan_info(_n.lib.hipsoxr_stream_plan(self._h), _C.byref(info)))
        # frames a constant-rate call can return at most: what the chunk adds plus what was pending before it
        self._slack = int((info.taps / 2 + 2) * self._ratio) + 4
        self._min_io = 1.0 / self._ratio  # (variable rate: the smallest io ratio requested so far bounds a call's output)
        self._arena, self._arena_off, self._arena_ptr, self._arena_stream = None, 0, 0, None
        self._esize = torch.empty(0, dtype=self.dtype).element_size()

    def __del__(self, _delete=_n.lib.hipsoxr_stream_delete):  # bound early: module globals may be gone at exit
        h = getattr(self, "_h", None)
        if h:
            _delete(h)
            self._h = None

    def clear(self):
        """Fresh signal: pending input and counters are dropped (reference: ResampleStream.clear)."""
        _n.check(_n.lib.hipsoxr_stream_clear(self._h))
        self._ended = False

    def delay(self):
        """Output frames still owed for the input fed so far (reference: ResampleStream.delay)."""
        return float(_n.lib.hipsoxr_stream_delay(self._h))

    def num_clips(self):
        """Integer outputs that saturated (reads a device counter: synchronises)."""
        return int(_n.lib.hipsoxr_stream_num_clips(self._h))

    def set_io_ratio(self, in_rate, out_rate, slew_len=0):
        """Variable-rate streams: move to in_rate / out_rate over slew_len output frames (reference:
        ResampleStream.set_io_ratio, src/soxr/__init__.py:162-179)."""
        if in_rate <= 0 or out_rate <= 0:
            raise ValueError("Sample rate should be over 0")
        io = float(in_rate) / float(out_rate)
        _n.check(_n.lib.hipsoxr_stream_set_io_ratio(self._h, io, int(slew_len)))
        self._min_io = min(self._min_io, io)

    def resample_chunk(self, x, last=False):
        import torch
        if self._ended:
            raise RuntimeError("Input after last input")
        if not x.is_cuda:
            raise RuntimeError("TensorStream needs device tensors (ResampleStream is the host-array surface)")
        if x.dtype != self.dtype:
            raise TypeError(f"Data type mismatch: stream is {self.dtype}, chunk is {x.dtype}")
        if x.ndim not in (1, 2) or (x.ndim == 1 and self.channels != 1) or (x.ndim == 2 and x.shape[1] != self.channels):
            raise ValueError("Input must be [frames] for one channel or [frames, channels]")
        if not x.is_contiguous():
            x = x.contiguous()
        ch, n = self.channels, int(x.shape[0])
        if self._vr:
            cap = int(_n.lib.hipsoxr_stream_delay(self._h) + n / self._min_io) + 4
        else:
            cap = int(n * self._ratio) + self._slack
        stream = torch.cuda.current_stream(x.device).cuda_stream
        fn, done = _n.lib.hipsoxr_stream_process_device, self._done
        if not last and cap <= 4096 and x.ndim == 1:
            # small mono chunks (the 10 ms case): results are carved out of an arena of 64 calls' worth — one tensor op (the
            # final view) per call instead of an allocation and a slice; a full arena is simply dropped (views keep it alive)
            # (an arena belongs to the HIP stream it was allocated on: a caller who moves to another stream gets a fresh one —
            #  the caching allocator may otherwise hand a dropped arena back to the first stream while this one still writes it.
            #  Results are VIEWS of the arena: keeping one 10 ms result alive keeps 64 calls' worth of HBM alive.)
            ar = self._arena
            if ar is None or self._arena_off + cap > ar.shape[0] or ar.device != x.device or self._arena_stream != stream:
                ar = self._arena = torch.empty(64 * cap, dtype=self.dtype, device=x.device)
                self._arena_off, self._arena_ptr, self._arena_stream = 0, ar.data_ptr(), stream
            off = self._arena_off
            optr = self._arena_ptr + off * self._esize
            err = fn(self._h, x.data_ptr() if n else optr, n, optr, cap, self._done_ref, stream)
            if err:
                _n.check(err)
            pos = done.value
            self._arena_off = off + ((pos + 7) & ~7)          # (16-byte steps for 2-byte samples: aligned views)
            return ar[off:off + pos]
        out = torch.empty((cap,) if x.ndim == 1 else (cap, ch), dtype=self.dtype, device=x.device)
        err = fn(self._h, x.data_ptr() if n else out.data_ptr(), n, out.data_ptr(), cap, self._done_ref, stream)
        if err:
            _n.check(err)
        pos = done.value
        if last:
            self._ended = True
            row = ch * x.element_size()
            while True:  # flush until the stream runs dry (src/soxr_ext.cpp:109-127)
                if pos >= out.shape[0]:
                    out = torch.cat([out, torch.empty_like(out)])
                _n.check(fn(self._h, None, 0, out.data_ptr() + pos * row, out.shape[0] - pos, self._done_ref, stream))
                if done.value == 0:
                    break
                pos += done.value
        return out[:pos]


class TensorStreamGroup:
    """N INDEPENDENT `TensorStream`s of one conversion served by ONE kernel launch per call (`hipsoxr_streams_process_device`):
    N live callers each feeding 10 ms chunks cost one dispatch per tick, whatever their phases and pending counts — the
    MI355X form of N threads around the reference's ResampleStream (src/soxr/__init__.py:56-131, tests/bench.py:71-88).

        grp = TensorStreamGroup(128, 44100, 16000, num_channels=1, dtype=torch.int16, quality="VHQ")
        y, counts = grp.resample_chunks(x)      # x: [128, frames] (mono) or [128, frames, channels]; stream i gets x[i]
                                                # y: [128, cap(, channels)]; stream i's frames are y[i, :counts[i]]

    Every stream is an ordinary stream handle: the frames stream i returns are those a `TensorStream` fed the same chunks
    returns, bit for bit; `streams[i]` IS such a TensorStream and may also be used alone (`grp.streams[i].resample_chunk`,
    `clear`, `delay`, ...).  Chunks of one call have one length (ragged feeding: call the streams singly, or pad by
    calling twice); variable-rate streams are not grouped."""

    def __init__(self, n, in_rate, out_rate, num_channels=1, dtype=None, quality="HQ", dither=True, dither_seeds=None):
        import torch
        if n < 1:
            raise ValueError("need at least one stream")
        self.streams = [TensorStream(in_rate, out_rate, num_channels, dtype, quality, False, dither,
                                     0 if dither_seeds is None else int(dither_seeds[i])) for i in range(n)]
        s0 = self.streams[0]
        self.n, self.channels, self.dtype = int(n), s0.channels, s0.dtype
        self._ratio, self._slack = s0._ratio, s0._slack
        self._handles = (_C.c_void_p * n)(*[s._h.value for s in self.streams])
        self._ins, self._outs = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        self._ilens, self._olens, self._dones = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        self._lane = np.arange(n, dtype=np.uint64)
        self._es = torch.empty(0, dtype=self.dtype).element_size()

    def resample_chunks(self, x):
        """x: [n_streams, frames] or [n_streams, frames, channels] device tensor -> (y, counts)."""
        import torch
        if not x.is_cuda or x.dtype != self.dtype:
            raise TypeError("TensorStreamGroup needs a device tensor of the group's dtype")
        if x.shape[0] != self.n or x.ndim not in (2, 3) or (x.ndim == 2 and self.channels != 1) or (x.ndim == 3 and x.shape[2] != self.channels):
            raise ValueError("Input must be [n_streams, frames] for one channel or [n_streams, frames, channels]")
        if any(s._ended for s in self.streams):
            raise RuntimeError("Input after last input")
        if not x.is_contiguous():
            x = x.contiguous()
        frames = int(x.shape[1])
        cap = int(frames * self._ratio) + self._slack
        y = torch.empty((self.n, cap) + tuple(x.shape[2:]), dtype=self.dtype, device=x.device)
        row = self.channels * self._es
        # a zero-frame tick: an empty tensor's data_ptr() is 0, and a NULL input is the C entry's "end of input" — point at
        # something non-null instead (nothing is read through it: ilens are 0), as TensorStream.resample_chunk does
        np.multiply(self._lane, np.uint64(frames * row), out=self._ins); self._ins += np.uint64(x.data_ptr() if frames else y.data_ptr())
        np.multiply(self._lane, np.uint64(cap * row), out=self._outs); self._outs += np.uint64(y.data_ptr())
        self._ilens[:] = frames
        self._olens[:] = cap
        stream = torch.cuda.current_stream(x.device).cuda_stream
        err = _n.lib.hipsoxr_streams_process_device(self._handles, self.n, self._ins.ctypes.data, self._ilens.ctypes.data,
                                                    self._outs.ctypes.data, self._olens.ctypes.data, self._dones.ctypes.data, stream)
        if err:
            _n.check(err)
        return y, self._dones.astype(np.int64)
