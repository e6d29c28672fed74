"""What `device` and `dist` share to describe a job to the library: the one place a `hipsoxr_job_t` is filled in (`make_job`),
the preamble of the raw clip-table entries (`table_job`), the clip table over tensors where they lie (`clip_table`) with its
batch check and packed offsets, and the way an entry is asked for its refusal (`refusal`).  Private to the package."""
import numpy as np

from . import _native as _n


def make_job(in_ptr, out_ptr, elem, kernel, n_clips, n_channels, in_strides, out_strides, in_frames, out_frames,
             in_abs0=0, out_k0=0, clip_counter=None, dither=False, dither_seed=0, clip_table=None, clip_table_dev=None):
    """A filled `hipsoxr_job_t`.  Pointers are ints or None; strides are (clip, frame, channel) in elements, or
    (frame, channel) for a clip stride of 0 (jobs over a clip table).  dither is taken as a truth value, dither_seed
    modulo 2^32."""
    j = _n.Job()
    j.in_, j.out, j.elem, j.kernel = in_ptr, out_ptr, elem, kernel
    j.n_clips, j.n_channels = n_clips, n_channels
    j.in_clip_stride, j.in_frame_stride, j.in_chan_stride = (0, *in_strides) if len(in_strides) == 2 else in_strides
    j.out_clip_stride, j.out_frame_stride, j.out_chan_stride = (0, *out_strides) if len(out_strides) == 2 else out_strides
    j.in_abs0, j.in_frames, j.out_k0, j.out_frames = in_abs0, in_frames, out_k0, out_frames
    j.clip_counter = clip_counter
    j.dither, j.dither_seed = bool(dither), int(dither_seed) & 0xFFFFFFFF
    if clip_table is not None or clip_table_dev is not None:  # (a fresh struct is zeroed; `Plan.run` passes neither)
        j.clip_table, j.clip_table_dev = clip_table, clip_table_dev
    return j


def table_job(table, io_ratios=None):
    """The preamble of a raw clip-table entry -> (rows, n_clips, in_frames, out_frames, ratios): the table as an int64
    [n_clips, 4] array, the job's extents (the maxima of its columns 1 and 3) and, where the entry takes a rate per clip,
    io_ratios as a float64 array of that length (else None).  The arrays are what the C call reads: the caller holds them
    until it returns."""
    t = np.ascontiguousarray(table, dtype=np.int64).reshape(-1, 4)
    r = None if io_ratios is None else np.ascontiguousarray(io_ratios, dtype=np.float64).reshape(-1)
    n = t.shape[0]
    if r is not None and r.shape[0] != n:
        raise ValueError("one io ratio per clip")
    if n == 0:  # (an empty array has no address worth passing: the entries refuse NULL tables)
        return np.zeros((1, 4), np.int64), 0, 0, 0, None if r is None else np.ones(1, np.float64)
    return t, n, int(t[:, 1].max()), int(t[:, 3].max()), r


def refusal(ask, *args, **kw):
    """What `ask(*args, **kw)` — a C entry given an empty job — refuses, as text, or None: so that a forward that could
    not be differentiated fails when it is called, not in the middle of backward."""
    try:
        ask(*args, **kw)
    except RuntimeError as e:
        return str(e)
    return None


def batch_check(clips):
    """-> (device, dtype, channels) of a non-empty list of clips that may share one job"""
    c0 = clips[0]
    ch = 1 if c0.ndim == 1 else c0.shape[1]
    for c in clips:
        if c.device != c0.device or c.dtype != c0.dtype or c.ndim not in (1, 2) or (1 if c.ndim == 1 else c.shape[1]) != ch:
            raise ValueError("clips of one job share device, dtype and channel count; each is [frames] or [frames, channels]")
    return c0.device, c0.dtype, ch


def packed_offsets(lengths, ch):
    """element offsets of clips of `lengths` frames laid end to end in a packed [sum(lengths), ch] buffer"""
    return np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int64) * ch


def table_rows(in_off, n_in, n_out, ch):
    """int64 table [n, 4] of rows (in_off[c], n_in[c], offset of clip c in the packed output, n_out[c])"""
    return np.ascontiguousarray(np.stack([in_off, n_in, packed_offsets(n_out, ch), n_out], axis=1), dtype=np.int64)


def clip_table(clips, n_other, ch, spare_ptr):
    """The table of a job that reads `clips` (checked tensors) WHERE THEY LIE and writes a packed buffer holding n_other[c]
    frames for clip c -> (base pointer, the tensors to keep alive, int64 table [n, 4]).  Rows are (offset from base in
    elements, frames, packed offset, n_other[c]); base is the lowest non-empty clip, or spare_ptr when every clip is
    empty."""
    keep = [c if c.is_contiguous() else c.contiguous() for c in clips]  # (a strided clip is the one case that is copied)
    es, n_own = keep[0].element_size(), [int(c.shape[0]) for c in keep]
    ptrs = [c.data_ptr() if n else None for c, n in zip(keep, n_own)]   # (an empty tensor has no storage address)
    base = min((p for p in ptrs if p is not None), default=spare_ptr)
    off = np.array([0 if p is None else (p - base) // es for p in ptrs], dtype=np.int64)
    return base, keep, table_rows(off, n_own, n_other, ch)
