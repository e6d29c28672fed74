/*
 * hipsoxr.h — native C ABI of the MI355X (gfx950) sample-rate converter.
 *
 * This is the drop-in boundary for the ONE hot path this repository accelerates:
 * libsoxr's constant-rate `soxr_process` underneath python-soxr's
 * `soxr.resample` / `ResampleStream.resample_chunk`.
 *
 * Every entry point names the reference interface it replaces (paths are relative to the
 * reference checkout, dofuuz/python-soxr):
 *
 *   hipsoxr_stream_create   <- soxr_create        call sites src/soxr_ext.cpp:76-78, :230-232, :305-307
 *   hipsoxr_stream_process  <- soxr_process       call sites src/soxr_ext.cpp:118-121, :163-166, :245-248,
 *                                                            :253-256, :328-331, :339-342
 *   hipsoxr_oneshot         <- soxr_oneshot       call site  src/soxr_ext.cpp:385-389
 *   hipsoxr_stream_delete   <- soxr_delete        src/soxr_ext.cpp:86, :260, :346
 *   hipsoxr_stream_clear    <- soxr_clear         src/soxr_ext.cpp:195
 *   hipsoxr_stream_delay    <- soxr_delay         src/soxr_ext.cpp:157, :191
 *   hipsoxr_stream_num_clips<- soxr_num_clips     src/soxr_ext.cpp:190
 *   hipsoxr_stream_engine   <- soxr_engine        src/soxr_ext.cpp:192
 *   hipsoxr_stream_set_io_ratio <- soxr_set_io_ratio src/soxr_ext.cpp:201
 *   hipsoxr_version         <- soxr_version       src/csoxr_version.cpp:6-8
 *   datatype / recipe constants <- soxr_datatype_t, SOXR_QQ..SOXR_VHQ  src/soxr_ext.cpp:32-46, :447-451
 *
 * Additions that have no counterpart in the reference (it has no GPU, no batch axis):
 *   hipsoxr_plan_*          the shared, immutable filter bank (what soxr_create designs per handle),
 *                           so that many streams / ranks share one bank (and RCCL can broadcast it);
 *   hipsoxr_run_device      device-pointer, batched, stateless launch of the hot path — the
 *                           entry the benchmark times (host-pointer soxr_process is PCIe-bound).
 *
 * Conventions (same as libsoxr): errors are static `const char *` strings, NULL == success;
 * handles are owned by the caller; input buffers are borrowed for the duration of the call and
 * fully consumed; output buffers are caller-allocated.  Distinct handles may be used concurrently
 * from different threads; one handle must not be.
 *
 * Plain C, no torch / HIP types in any signature (streams are passed as `void *` = hipStream_t).
 */
#ifndef HIPSOXR_H
#define HIPSOXR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HIPSOXR_API __attribute__((visibility("default")))

typedef const char *hipsoxr_error_t; /* NULL == success (reference: src/soxr_ext.cpp:80-82) */

/* Same numbering as libsoxr's soxr_datatype_t (reference: src/soxr_ext.cpp:35-46). */
typedef enum {
    HIPSOXR_FLOAT32_I = 0, /* interleaved [frame][channel] */
    HIPSOXR_FLOAT64_I = 1,
    HIPSOXR_INT32_I = 2,
    HIPSOXR_INT16_I = 3,
    HIPSOXR_FLOAT32_S = 4, /* split: one contiguous buffer per channel */
    HIPSOXR_FLOAT64_S = 5,
    HIPSOXR_INT32_S = 6,
    HIPSOXR_INT16_S = 7
} hipsoxr_datatype_t;

/* Quality recipes — libsoxr values (reference: src/soxr_ext.cpp:447-451). */
#define HIPSOXR_QQ 0UL
#define HIPSOXR_LQ 1UL
#define HIPSOXR_MQ 2UL
#define HIPSOXR_HQ 4UL
#define HIPSOXR_VHQ 6UL

/* Stream flags. */
#define HIPSOXR_VR 32UL        /* quality-spec flag: variable rate (reference: src/soxr_ext.cpp:74) */
#define HIPSOXR_NO_DITHER 8UL  /* io-spec flag: disable int16 TPDF dither */
#define HIPSOXR_DEFER 64UL     /* (extension) deferred output: a process call enqueues its work and returns the
                                  PREVIOUS call's frames — no GPU round trip inside the call.  Same concatenated
                                  output; frames surface one call later (the reference's contract allows any
                                  per-call count, README.md:77-78).  Constant-rate interleaved streams. */
#define HIPSOXR_RESIDENT 128UL /* (extension) synchronous small chunks (results <= 2048 frames, ring in pinned host
                                  memory) are served by a kernel that STAYS on the GPU between calls and is fed
                                  through a mailbox in pinned memory: no HIP call per chunk, ~3x lower latency
                                  per call.  Same output, bit for bit.  The kernel leaves by itself after
                                  HIPSOXR_RESIDENT_IDLE_US (default 1000) without a call; until then device-wide
                                  synchronisations elsewhere in the process wait for it.  Interleaved streams,
                                  constant or variable rate (a variable-rate message carries its own Q64.64
                                  clock), without HIPSOXR_DEFER.  Also: environment HIPSOXR_RESIDENT. */
#define HIPSOXR_AUTO_RESIDENT 256UL /* (extension, opt-in; also environment HIPSOXR_AUTO_RESIDENT) the stream turns the
                                  resident path on BY ITSELF once it has been fed 16 small chunks back to back (each
                                  within 500 us of the one before) and off again at the first call that breaks the run;
                                  such instances may hold at most an eighth of the chip.  Not a default: while a
                                  resident kernel spins, hipDeviceSynchronize / hipFree anywhere in the process wait
                                  until it leaves (up to the idle time, longer if another thread keeps feeding it). */
#define HIPSOXR_STREAM_FFT 512UL /* (extension, opt-in) every emission of the stream runs on the frequency-domain engine
                                  (HIPSOXR_KERNEL_FFT's, 2-3x faster than the canonical order on chunks of seconds of
                                  audio) instead of the canonical-order kernels: same frame counts per call, same delay
                                  and flush behaviour, values 1e-6-class (integers within 1 LSB) — NOT bit-identical to
                                  the default stream or to another cut of the same signal into chunks.  For
                                  hipsoxr_stream_process_device only (host-pointer and grouped calls on such a handle
                                  are an error).  Refused at creation, by name, where the engine cannot serve the
                                  stream: variable rate, ratios without an exact bank or outside the engine's schedule
                                  table, recipes below HQ, split layouts, HIPSOXR_DEFER / _RESIDENT / _AUTO_RESIDENT,
                                  int32 with more than one channel, int16 with an odd channel count above one. */

/* Element types used by device jobs (layout is given by strides, not by the type). */
typedef enum {
    HIPSOXR_F32 = 0, HIPSOXR_F64 = 1, HIPSOXR_I32 = 2, HIPSOXR_I16 = 3,
    /* IEEE binary16 and bfloat16 samples, DEVICE JOBS ONLY (hipsoxr_run_device, hipsoxr_run_device_adjoint): input and output
     * have the same type, the arithmetic is float32 throughout.  The result is, bit for bit, the HIPSOXR_F32 job of the same
     * selector and layout on the exactly widened samples, followed by ONE round-to-nearest-even conversion: NaN stays NaN,
     * +-inf stays +-inf, a float32 result beyond the type's range becomes +-inf (no saturation), float16 subnormals are exact
     * on the way in and correctly rounded on the way out; dither and clip_counter are ignored, as for float jobs.  Where the
     * float32 job runs the frequency-domain engine's paired kernels on unit-stride columns or interleaved channel pairs (and
     * under a clip_table: unit-stride columns, one ragged launch) the conversion is fused into that kernel — 2-byte loads,
     * 16-byte stores of eight samples; everywhere else (small jobs, recipes below HQ, ratios outside the schedule table,
     * interpolated-phase plans, other layouts, HIPSOXR_KERNEL_EXACT / _GATHER / _TILE*, job windows, the adjoint entry) the
     * job is one widening pass into stream-ordered float32 temporaries packed in the caller's dimension order, the float32
     * job, and one narrowing pass that writes exactly the job's output elements (ranges of clips — with one clip, of
     * channels — keep the temporaries of a range at or below 1 GiB; each range is then the float32 job of that range).
     * One difference in engine choice: 44.1k -> 48k from 8192 block pairs, where float32 takes the one-wave kernel, stays
     * on the fused paired kernel (1e-6 class either way).  A clip_table the fused path does not take runs clip by clip.
     * Refused by name: HIPSOXR_KERNEL_FFT_PCM, _FFT_F64 and _WAVE_DOT on these types, hipsoxr_run_device_adjoint_ragged,
     * and every stream entry — hipsoxr_datatype_t has no such member (its values 4 and 5 are the split float layouts, and a
     * stream reads them as that). */
    HIPSOXR_F16 = 4, HIPSOXR_BF16 = 5
} hipsoxr_elem_t;

/* Kernel selector for hipsoxr_run_device. */
typedef enum {
    HIPSOXR_KERNEL_AUTO = 0,   /* fastest admissible engine, including the FFT engine for large float jobs
                                  (integer jobs: always the canonical-order kernels, bit for bit) */
    HIPSOXR_KERNEL_GATHER = 1, /* one lane per output sample, operands gathered through L1/L2 */
    HIPSOXR_KERNEL_TILE = 2,   /* period-tiled, best variant for the engine (MFMA f32, else VALU) */
    HIPSOXR_KERNEL_TILE_VALU = 3, /* period-tiled: input slab in LDS, coefficients on the scalar path */
    HIPSOXR_KERNEL_TILE_MFMA = 4, /* period-tiled on the f32-input matrix pipe (f32 engine only) */
    HIPSOXR_KERNEL_FFT = 5,    /* frequency-domain overlap-save engine (whole-signal float32 jobs; 1e-6-class,
                                  not bit-identical to the canonical order) */
    HIPSOXR_KERNEL_EXACT = 6,  /* AUTO restricted to the canonical-order kernels (bit-exact invariances) */
    HIPSOXR_KERNEL_WAVE_DOT = 7, /* reference point only: one wavefront per output sample + shuffle reduction
                                  (the shape BASELINE.json's north star describes); 64-way tree order, so
                                  1e-6-class like FFT, never chosen automatically */
    HIPSOXR_KERNEL_FFT_F64 = 8, /* the frequency-domain engine computing in float64 whatever the I/O type: float32
                                  jobs at the width libsoxr's VHQ recipe itself computes in (its float64 engine;
                                  reference src/soxr_ext.cpp:74,228 pass the recipe through unchanged) — results
                                  differ from the float64 direct form by the float32 OUTPUT rounding only
                                  (~3e-8 relative RMS).  Unit-stride columns of the tabled ratios. */
    HIPSOXR_KERNEL_FFT_PCM = 9  /* the frequency-domain engine on int16 / int32 device jobs: int16 in float32 arithmetic,
                                  int32 in float64 (the exact engine's widths), samples in LSB units, then the exact
                                  engine's own output stage — dither (job.dither, job.dither_seed), round half to even,
                                  saturate, job.clip_counter.  Opt-in by name only: integer results are within 1 LSB
                                  of the canonical order, not bit-identical, and AUTO keeps integers on the exact
                                  engine.  Whole signals on HQ / VHQ plans of the tabled ratios; unit-stride columns
                                  (ragged batches included) and int16 interleaved channel pairs; float jobs and
                                  anything else it cannot serve are an error, never a run of another engine. */
} hipsoxr_kernel_t;
/* Selector of hipsoxr_run_device_adjoint alone (job.kernel there; the forward entries refuse it by name), numbered on from
 * hipsoxr_kernel_t. */
typedef enum {
    HIPSOXR_KERNEL_ADJOINT = 10, /* hipsoxr_run_device_adjoint (and its _ragged form) only: the exact engine's transposed operator for EVERY
                                  constant-rate plan.  On an exact-bank plan it runs what AUTO runs there, bit for bit; on an
                                  interpolated-phase plan (hipsoxr_plan_info_t::interpolated != 0, which AUTO and EXACT
                                  refuse) the gather-form adjoint on the plan's own interpolation table — the coefficients
                                  the forward's HIPSOXR_KERNEL_EXACT multiplies by, to the bit.  float32 / float64, whole
                                  signals, a clip_table on the _ragged entry alone, constant-rate plans (not hipsoxr_plan_create_vr's); refused by
                                  name otherwise, and on hipsoxr_run_device. */
    HIPSOXR_KERNEL_ADJOINT_FFT = 11, /* the same two entries only: the transposed operator on the FREQUENCY-DOMAIN engine, for
                                  exact-bank HQ / VHQ plans.  gx = A^T gy is computed as the forward float job of the plan's
                                  transposed plan (L' = M, M' = L, the prototype mirrored: the same float64 coefficients) on the
                                  kernels HIPSOXR_KERNEL_FFT runs — so it is in that engine's class, 1e-6 (float32) / 2e-9 VHQ,
                                  1e-6 HQ (float64) relative RMS, not bit-identical to the exact adjoint, at about the
                                  forward engine's cost for the reversed ratio.  float32 / float64 (HIPSOXR_F16 / _BF16 on the
                                  equal-length entry: the float32 job on the widened cotangent, rounded once), whole
                                  signals, every layout the engine serves for the reversed ratio, a clip_table on the _ragged
                                  entry (one launch).  Opt-in by name only: AUTO and EXACT keep the exact adjoint, bit for bit.
                                  Refused by name: integer types, variable-rate and interpolated-phase plans, recipes below
                                  120 dB, in_abs0 / out_k0 != 0, a clip_table on the equal-length entry or none on the ragged
                                  one; where the engine has no form for the plan or layout the call fails ("unavailable") —
                                  it never runs the exact adjoint instead.  No new field, no new entry. */
    HIPSOXR_KERNEL_ADJOINT_TWO_STAGE = 12, /* hipsoxr_run_device_adjoint only: the transposed TWO-STAGE FORM, for the interpolated-phase
                                  HQ / VHQ plans (arbitrary ratios: 48000 -> 44101, float rates) whose float forward AUTO runs on
                                  that form.  gx = A^T gy with A the forward job the form runs for (in_frames = n_x, out_frames =
                                  n_y), transposed stage by stage around the same intermediate window: the FFT stage's
                                  transposed plan (1:2 <-> 2:1) on the kernels HIPSOXR_KERNEL_FFT runs, and k_poly_adj, the
                                  gather-form transpose of the polyphase stage on the forward's own cubic table and position
                                  arithmetic — no atomics, bitwise reproducible, at about the forward form's cost where
                                  HIPSOXR_KERNEL_ADJOINT walks the plan's full tap count with a cubic per tap.  In the form's
                                  class against the exact adjoint: 1e-6 (float32) / 2e-9 VHQ, 1e-6 HQ (float64) relative RMS.
                                  float32 / float64 (HIPSOXR_F16 / _BF16: the float32 job on the widened cotangent, rounded
                                  once), whole cotangents, any clips x channels and strides.  Opt-in by name only.  Refused by
                                  name: integer types, variable-rate plans, exact-bank plans (HIPSOXR_KERNEL_ADJOINT_FFT serves
                                  those), in_abs0 / out_k0 != 0, a clip_table, and the _ragged entry (clip tables are not served
                                  yet); a plan without the form (below HQ, a bank installed from outside, steeper than 4:1), a
                                  job it does not admit (fewer than 8192 frames either side, too many columns, LDS) or an FFT
                                  stage that declines fails ("unavailable", naming HIPSOXR_KERNEL_ADJOINT as the exact
                                  alternative) — it never runs the exact adjoint instead.  No new field, no new entry. */
    HIPSOXR_KERNEL_ADJOINT_AUTO = 13 /* hipsoxr_run_device_adjoint and hipsoxr_run_device_adjoint_ragged only: the TRANSPOSE OF THE
                                  JOB THE FORWARD LAUNCHES UNDER HIPSOXR_KERNEL_AUTO for the same plan and shape — the selector that
                                  picks a fast gradient where there is one and never answers "unavailable".  Exact-bank plan:
                                  the frequency-domain engine (HIPSOXR_KERNEL_ADJOINT_FFT's launch) when the forward's outputs in
                                  all — cotangent frames over clips or rows, times channels — reach 8192 on an HQ / VHQ plan and
                                  the engine takes the transposed plan, else the exact adjoint.  Interpolated-phase plan, equal
                                  lengths: the transposed two-stage form (HIPSOXR_KERNEL_ADJOINT_TWO_STAGE's launch) when the
                                  plan has the form, the job is admitted (8192 frames either side) and the FFT stage accepts,
                                  else k_adj_interp.  Interpolated-phase plan, clip table: per clip — a clip the form admits
                                  alone runs on it (k_poly_adj's ragged instance and the FFT stage's transposed plan over the
                                  table's columns: a constant number of launches per range of at most 1 GiB of intermediate),
                                  every other clip in ONE ragged launch of the exact adjoint, a clip with n_x == 0 writes
                                  nothing; each clip's engine, and on the exact adjoint its bits, are those of the clip alone.
                                  HIPSOXR_NO_FFT / HIPSOXR_NO_TWO_STAGE send it to the exact adjoint as they send AUTO's forward
                                  to the exact engine.  Where it resolves to a named selector the bits are that selector's.
                                  Refused by name, as under HIPSOXR_KERNEL_ADJOINT: integer types, variable-rate plans, in_abs0 /
                                  out_k0 != 0, a clip_table on the equal-length entry and none on the ragged one, HIPSOXR_F16 /
                                  _BF16 on the ragged entry (the equal-length entry widens them), rows above the plan's output
                                  length.  HIPSOXR_KERNEL_AUTO / _EXACT on these entries keep their meaning and their bits. */
} hipsoxr_adjoint_kernel_t;

typedef struct hipsoxr_plan hipsoxr_plan_t;     /* immutable: ratio + polyphase bank (host + device) */
typedef struct hipsoxr_stream hipsoxr_stream_t; /* stateful converter: the `soxr_t` counterpart */

/* ---- library ---------------------------------------------------------------------------- */
#define HIPSOXR_VERSION_STRING "0.7.0" /* one number for hipsoxr_version() and the libsoxr-named soxr_version() */
HIPSOXR_API const char *hipsoxr_version(void);
HIPSOXR_API int hipsoxr_device_count(void); /* 0 when no HIP device is visible (never throws) */

/* ---- plan: what soxr_create designs (filter bank for in_rate -> out_rate at a recipe) ---- */
typedef struct {
    double in_rate, out_rate;
    unsigned long recipe;
    int64_t L, M;          /* out/in = L/M in lowest terms: L phases, phase step M              */
    int32_t taps;          /* taps per phase (even, multiple of 8)                               */
    int32_t interpolated;  /* 0: exact rational bank [L][taps]; P > 0: interpolated-phase plan
                              (ratios whose exact bank would exceed 2^22 entries): the bank is the
                              cubic coefficient table [P][taps][4]                               */
    double precision_bits; /* 0 (QQ), 16, 20, 28                                                 */
    double passband_end;   /* fraction of the lower rate's Nyquist                                */
    double stopband_begin;
    double att_db;         /* design stop-band attenuation                                        */
    double kaiser_beta;
    uint64_t bank_elems;   /* L * taps, or P * taps * 4                                           */
} hipsoxr_plan_info_t;

HIPSOXR_API hipsoxr_error_t hipsoxr_plan_create(double in_rate, double out_rate,
                                                unsigned long recipe, hipsoxr_plan_t **out);
/* The plan a variable-rate stream created with the same arguments uses (always an interpolated-phase
 * table, designed for the largest io ratio in_rate/out_rate; reference: src/soxr_ext.cpp:74).  Host only. */
HIPSOXR_API hipsoxr_error_t hipsoxr_plan_create_vr(double in_rate, double out_rate,
                                                   unsigned long recipe, hipsoxr_plan_t **out);
HIPSOXR_API void hipsoxr_plan_delete(hipsoxr_plan_t *);
HIPSOXR_API hipsoxr_error_t hipsoxr_plan_info(const hipsoxr_plan_t *, hipsoxr_plan_info_t *info);
/* Copy the float64 bank (phase-major [L][taps], or [P][taps][4]) into dst (n = bank_elems doubles). */
HIPSOXR_API hipsoxr_error_t hipsoxr_plan_get_bank(const hipsoxr_plan_t *, double *dst, size_t n);
/* Replace the bank (e.g. with the one RCCL-broadcast from rank 0); device tables are rebuilt. */
HIPSOXR_API hipsoxr_error_t hipsoxr_plan_set_bank(hipsoxr_plan_t *, const double *src, size_t n);
/* Multi-GPU: broadcast the bank from rank `root` to every rank of an RCCL communicator (`nccl_comm` is an
 * ncclComm_t; one process per GPU, each calls this with its own plan created from the same arguments;
 * `my_rank` is the caller's rank in the communicator).  Ranks other than root install what they receive
 * (device tables rebuild on next use).  This is the only collective of the path: clips shard across
 * ranks with no data-path exchange (BASELINE.json north_star: "RCCL broadcast of the shared filter bank
 * over xGMI").  RCCL is looked up in the running process (e.g. PyTorch's copy), else dlopen'ed. */
HIPSOXR_API hipsoxr_error_t hipsoxr_plan_broadcast(hipsoxr_plan_t *, void *nccl_comm, int root, int my_rank,
                                                   void *hip_stream);
/* Total output frames for `in_len` input frames: floor(in_len*L/M + 1/2). */
HIPSOXR_API uint64_t hipsoxr_plan_out_len(const hipsoxr_plan_t *, uint64_t in_len);

/* ---- device job: the hot path on device-resident buffers (batched, stateless) ------------- */
typedef struct {
    const void *in;  /* device pointer */
    void *out;       /* device pointer */
    int32_t elem;    /* hipsoxr_elem_t of in and out */
    int32_t kernel;  /* hipsoxr_kernel_t */
    uint32_t n_clips, n_channels;
    /* strides in ELEMENTS: address(clip, frame, ch) = base + clip*cs + frame*fs + ch*chs */
    int64_t in_clip_stride, in_frame_stride, in_chan_stride;
    int64_t out_clip_stride, out_frame_stride, out_chan_stride;
    int64_t in_abs0;   /* absolute stream index of in[frame 0] (0 for a whole signal)            */
    int64_t in_frames; /* frames present at `in`; the signal is zero outside [in_abs0, +frames)  */
    int64_t out_k0;    /* absolute index of the first output frame to produce                    */
    int64_t out_frames;/* output frames to produce (per clip)                                    */
    /* Window jobs (in_abs0 / out_k0 != 0) on the exact engine are tested bit for bit — against the oracle at the job's own
     * position and against the same job moved down by whole periods — with out_k0 up to 2^50 and in_abs0 to match, across
     * 2^31 and 2^32 on either side (tests/test_gpu_window_positions.py).  hipsoxr_run_device refuses a negative out_k0
     * ("invalid job extent").  A negative in_abs0 is not refused — in[0] then lies in front of stream index 0, which the
     * two-stage form uses internally on the frequency-domain engine — but no caller-facing test covers it. */
    uint64_t *clip_counter; /* device counter of saturated integer outputs, or NULL            */
    uint32_t dither;        /* 1: TPDF dither on int16 output                                    */
    uint32_t dither_seed;
    /* Ragged batches — independent clips of unequal length in ONE job (what a corpus is: the reference takes any
     * length per call, src/soxr/__init__.py:182-231).  NULL: every clip has in_frames / out_frames and starts at
     * clip * clip_stride.  Else n_clips rows of four int64 { in_offset, in_frames, out_offset, out_frames }, offsets in
     * ELEMENTS from `in` / `out` (clip c, frame f, channel ch is at in + in_offset[c] + f*in_frame_stride +
     * ch*in_chan_stride; the clip strides are ignored), out_frames[c] <= hipsoxr_plan_out_len(in_frames[c]).
     * clip_table is in HOST memory and is what the library validates (counts against the job and the plan; the
     * caller guarantees that offset + extent stays inside its buffers — the library does not know their sizes).
     * clip_table_dev is optional: NULL = the library uploads the host table itself, in stream order, on every call
     * (~10 us); a device copy supplied by the caller (a prepared job launched many times) is used as it is and must
     * equal the host table — it is not checked.  in_frames / out_frames of the job are then the LARGEST per-clip
     * values.  Whole signals only (in_abs0 == 0, out_k0 == 0).  Unit-stride float columns go out as one launch of
     * the frequency-domain engine (AUTO: from 2^13 output samples in all, as for equal-length jobs).  Interleaved and
     * strided clips (frame strides other than 1: [frames, channels] tensors, channel slices) are one launch of that
     * engine BY NAME — HIPSOXR_KERNEL_FFT on float32 / float64 (channel pairs for even channel counts, single strided
     * columns otherwise; at most 65535 clips per launch of the paired form), HIPSOXR_KERNEL_FFT_PCM on int16 with an even
     * channel count whose rows' two offsets are even (one aligned 4-byte word per frame and channel pair; the dither key is
     * the output index within the clip) — while HIPSOXR_KERNEL_AUTO keeps such tables on the exact engine, bit for bit.
     * Still refused by name: HIPSOXR_KERNEL_FFT_F64 on strided float32 data, int32 channel pairs, int16 with an odd channel
     * count or at an odd offset, ratios outside the schedule table; float16 / bfloat16 interleaved tables run clip by clip.
     * Everything else on
     * an exact-bank plan is ONE launch of the exact engine too: int16 / int32 under the default selector, interleaved
     * or float64 clips under AUTO, small jobs, HIPSOXR_KERNEL_EXACT and the tile / gather selectors — the kernel reads its clip's
     * row, the grid is the longest clip's (more than 65535 columns: one launch per range of clips).  Each clip has the
     * bits of the clip run alone; out[0, out_frames[c]) of every clip is written and nothing else, not the elements
     * between packed clips either; clip_counter receives the sum over the clips.  An interpolated-phase plan (an
     * arbitrary ratio) is ONE launch in the same way — int16 / int32 under the default selector, every type under
     * HIPSOXR_KERNEL_EXACT / HIPSOXR_KERNEL_GATHER — on the ragged forms of its own kernels, each clip with the bits of
     * the clip run alone.  float32 / float64 clips of such a plan under HIPSOXR_KERNEL_AUTO belong to the two-stage
     * form (another precision class), and a table at any positive frame stride (mono clips, planar channels at any
     * channel stride, interleaved [frames, channels] clips, channel slices) is a CONSTANT number of launches whatever the
     * number of clips: the table is
     * partitioned by the question asked of each clip alone — a clip of 8192 frames or more on both sides that the form
     * admits runs the two-stage form, every other non-empty clip the exact engine, so engine choice per clip does not
     * depend on the table — into one ragged polyphase launch and one ragged FFT-stage launch over the (clip, channel)
     * columns of the admitted clips, and one ragged launch of the interpolated kernels over the others.  Only two cuts
     * multiply that: more than 65535 admitted columns, or more than 1 GiB of intermediate signal (each range of columns
     * is one stream-ordered allocation, one launch pair and one free).  Precision: admitted clips are within the two-stage
     * class of the float64 direct form (1e-6 float32, 2e-9 float64, relative RMS), NOT bit-equal to the clip run alone (a
     * mono float32 clip alone takes another kernel form of the polyphase stage: other rounding, same class); the short
     * clips ARE bit-equal to the clip alone.  The inner launches read tables the library derives (columns, offsets into the
     * intermediate; one upload per call), so clip_table_dev cannot serve this path and is not read by it.
     * With a frame stride other than 1 both stages run one column per (clip, channel) at the caller's stride on the
     * caller's side (the intermediate stays library-owned and unit-stride); the results are in the same class.
     * Served clip by clip from the same call, same results: HIPSOXR_KERNEL_WAVE_DOT, and a table with a clip of more
     * than 2^30 outputs.  HIPSOXR_KERNEL_FFT / _FFT_F64 on a table of an interpolated-phase plan stay refused. */
    const int64_t *clip_table;
    const int64_t *clip_table_dev;
} hipsoxr_job_t;
/* ZERO-INITIALISE the struct (memset / = {0}) before filling it: fields are only ever APPENDED, a zero field always
 * means "feature not used", and hipsoxr_version() changes when one is added (0.1: up to dither_seed; 0.3: clip_table,
 * clip_table_dev; 0.6: no new field — the kernel selector HIPSOXR_KERNEL_FFT_PCM; 0.7: no new field — the stream flag HIPSOXR_STREAM_FFT; no new field — the selector HIPSOXR_KERNEL_ADJOINT; no new field — the entry hipsoxr_run_device_adjoint_ragged; no new field, no new entry — a clip_table on the exact engine is one launch; no new field, no new entry — a float clip_table of an interpolated-phase plan is a constant number of launches of the two-stage form; no new field — the element types HIPSOXR_F16 / HIPSOXR_BF16; no new field — the entries hipsoxr_plan_vr_out_len and hipsoxr_run_device_vr_ragged; no new field — the selector HIPSOXR_KERNEL_ADJOINT_FFT).  A client compiled against an older header must not be run against a newer struct-consuming
 * library without recompiling — check the version string at load time as soxr_amd/_native.py does. */

/* Enqueue the job on `hip_stream` (a hipStream_t; NULL = default stream). Asynchronous. */
HIPSOXR_API hipsoxr_error_t hipsoxr_run_device(hipsoxr_plan_t *, const hipsoxr_job_t *job,
                                               void *hip_stream);
/* gx = A^T gy for the forward job A that hipsoxr_run_device(HIPSOXR_KERNEL_EXACT) computes on the same plan: the transposed
 * polyphase operator on the same bank (the gradient of a resample; the adjoint an iterative solver needs).  The job is read in
 * the adjoint's own direction: `in` is gy with in_frames = n_y frames, `out` is gx with out_frames = n_x frames, strides as
 * usual; in_frames <= hipsoxr_plan_out_len(plan, out_frames) (a truncated forward output has a truncated cotangent).  Every
 * element of gx is written (0 where no output reads the input), nothing outside it; gather form, no atomics: results are
 * bitwise reproducible and independent of layout.  HIPSOXR_F32 / HIPSOXR_F64 (HIPSOXR_F16 / HIPSOXR_BF16: the float32 adjoint on
 * the widened cotangent, rounded once) on exact-bank plans; kernel = HIPSOXR_KERNEL_AUTO
 * or _EXACT; in_abs0 == 0, out_k0 == 0, clip_table == NULL; anything else is an error that names the reason, never a run of
 * another path.  kernel = HIPSOXR_KERNEL_ADJOINT: the same on every constant-rate plan, interpolated-phase plans included
 * (A is then the forward HIPSOXR_KERNEL_EXACT computes from the plan's interpolation table).  Zero frames, clips or channels: success, nothing launched.  Asynchronous on `hip_stream`. */
HIPSOXR_API hipsoxr_error_t hipsoxr_run_device_adjoint(hipsoxr_plan_t *, const hipsoxr_job_t *job, void *hip_stream);
/* The same operator over a RAGGED batch — clips of unequal length, ONE launch: the gradient of a hipsoxr_run_device job that
 * has a clip_table.  The job is read in the adjoint's direction as above, and clip_table is REQUIRED: n_clips host rows
 * { gy offset, n_y, gx offset, n_x }, offsets in elements from `in` / `out` (the clip strides are ignored), n_y[c] <=
 * hipsoxr_plan_out_len(plan, n_x[c]); in_frames / out_frames of the job are the LARGEST per-clip n_y / n_x.  clip_table_dev
 * follows the forward's rule: NULL = the host table is uploaded in stream order on every call, a caller's device copy is
 * used as it is and must equal the host table.  Every element of every clip's gx[0, n_x[c]) is written (zeros where
 * n_y[c] == 0), nothing outside it — not the elements between packed clips either.  Each clip has, bit for bit, the result
 * of the same clip run alone through hipsoxr_run_device_adjoint (finite cotangents; a non-finite gy[k] reaches, inside its
 * own clip only, what it reaches in the kernel form the ragged launch took).  Selectors: HIPSOXR_KERNEL_AUTO, _EXACT (exact-bank
 * plans) and HIPSOXR_KERNEL_ADJOINT (every constant-rate plan).  Refused by name, before anything is launched: a NULL
 * clip_table, a negative offset or count, a row above the job's in_frames / out_frames, n_y[c] above the plan's output length
 * for n_x[c], integer element types, HIPSOXR_F16 / HIPSOXR_BF16, in_abs0 / out_k0 != 0, variable-rate plans, any other selector.  No clips, no channels
 * or out_frames == 0: success, nothing launched.  Asynchronous on `hip_stream`. */
HIPSOXR_API hipsoxr_error_t hipsoxr_run_device_adjoint_ragged(hipsoxr_plan_t *, const hipsoxr_job_t *job, void *hip_stream);

/* ---- per-clip rates: a ragged batch on a variable-rate plan (speed perturbation in one launch) ---- */
/* Outputs of `in_len` frames at constant io ratio `io_ratio` on a variable-rate plan (what a variable-rate stream set to that
 * ratio before its first input emits in all: the k >= 0 with k S + S/2 <= in_len 2^64, S the ratio's truncated Q64.64 step);
 * 0 on a plan that is not variable-rate, and for a ratio hipsoxr_stream_set_io_ratio would refuse on it.  Host only. */
HIPSOXR_API uint64_t hipsoxr_plan_vr_out_len(const hipsoxr_plan_t *, uint64_t in_len, double io_ratio);
/* A ragged batch in which clip c is resampled at io_ratios[c] (input frames per output frame), all clips in ONE launch of the
 * exact engine's variable-rate kernels (more than 65535 clip x channel columns: one launch per range of clips).  The plan is
 * hipsoxr_plan_create_vr's: one interpolated-phase table designed for the LARGEST io ratio, in_rate / out_rate; every
 * smaller ratio is a step on the same table (no filter design and no upload per ratio).  The job is read as a ragged forward
 * job: clip_table is REQUIRED — n_clips host rows { in offset, n_in, out offset, n_out } in elements from `in` / `out`, the
 * clip strides are ignored, in_frames / out_frames are the LARGEST per-clip counts, frame and channel strides as usual
 * (unit-stride columns, interleaved [frames, channels], strided); clip_table_dev as on ragged jobs (NULL: uploaded in stream
 * order).  io_ratios is a HOST array of n_clips doubles, read before the call returns; io_ratios[c] becomes the clip's step
 * by the truncation hipsoxr_stream_set_io_ratio applies.
 * Clip c has, BIT FOR BIT, the frames that a fresh variable-rate stream of this plan — same type, channel count, dither
 * flag and seed — yields when it is given hipsoxr_stream_set_io_ratio(s, io_ratios[c], 0) before any input, fed the whole
 * clip and flushed, truncated to n_out[c] <= hipsoxr_plan_vr_out_len(plan, n_in[c], io_ratios[c]).  int16 dither is keyed by
 * (seed, channel, output index within the clip); clip_counter receives the sum of those streams' counts.  Nothing outside
 * a clip's [0, n_out[c]) is written, not the elements between packed clips either.
 * Selectors: HIPSOXR_KERNEL_AUTO, _EXACT and _GATHER all run this one launch (no 1e-6-class form of it exists: AUTO is
 * bit-exact here for floats too).  float32, float64, int32, int16.
 * Refused by name, before anything is launched: a plan not made by hipsoxr_plan_create_vr, a NULL clip_table or io_ratios,
 * a ratio outside (2^-20, 2^20) or above the plan's in_rate / out_rate (by more than the factor 1 + 1e-12 that
 * hipsoxr_stream_set_io_ratio allows, in its words), a negative offset or count, a row above the job's in_frames /
 * out_frames, n_out[c] above hipsoxr_plan_vr_out_len, a clip of more than 2^30 outputs, in_abs0 / out_k0 != 0, HIPSOXR_F16 /
 * HIPSOXR_BF16, any other selector.  Not served: a ratio change inside a clip (streams have slews), the
 * frequency-domain engine.  Gradients: hipsoxr_run_device_vr_ragged_adjoint, below.  No clips, no channels or
 * out_frames == 0: success, nothing launched.  Asynchronous on `hip_stream`. */
HIPSOXR_API hipsoxr_error_t hipsoxr_run_device_vr_ragged(hipsoxr_plan_t *, const hipsoxr_job_t *job,
                                                         const double *io_ratios /* host, n_clips */, void *hip_stream);
/* The gradient of that launch — gx[c] = A_c^T gy[c] for every clip of a clip table, ONE launch whatever the number of clips:
 * A_c is the forward hipsoxr_run_device_vr_ragged computes for n_x[c] input frames at io_ratios[c], truncated to its first
 * n_y[c] outputs.  The job is read in the adjoint's direction, as hipsoxr_run_device_adjoint_ragged reads it: `in` is gy,
 * `out` is gx, clip_table is REQUIRED — n_clips host rows { gy offset, n_y, gx offset, n_x } in elements from `in` / `out`
 * (the clip strides are ignored), in_frames / out_frames the LARGEST per-clip n_y / n_x, clip_table_dev as on ragged jobs.
 * io_ratios is a HOST array of n_clips doubles, read before the call returns and turned into steps as on the forward.
 * The coefficient of gy[k] in gx[a] is the very value the forward multiplies x[a] by for output k (the plan's interpolation
 * table, the same integer position arithmetic, the same fma nesting); every gx[a] is one fma chain over ascending k from +0
 * in the element's width, at most ceil(taps / io ratio) + 1 terms.  Gather form, no atomics: bitwise reproducible, and each
 * clip has the bits of the same clip run alone.  Every element of every clip's gx[0, n_x[c]) is written (+0 where no output
 * reads the frame, all of a clip with n_y[c] == 0), nothing outside it — not the elements between packed clips either.  A
 * non-finite gy[k] reaches the frames of its true support, q_k - (taps/2 - 1) .. q_k + taps/2 with q_k = (k S) >> 64, and
 * nothing else.  HIPSOXR_F32 / HIPSOXR_F64.  Selectors: HIPSOXR_KERNEL_AUTO and HIPSOXR_KERNEL_ADJOINT, the same launch and
 * the same bits.
 * Refused by name, before anything is launched: a plan not made by hipsoxr_plan_create_vr, a NULL clip_table or io_ratios, a
 * ratio the forward entry refuses (in its words), a negative offset or count, a row above the job's in_frames / out_frames,
 * n_y[c] above hipsoxr_plan_vr_out_len(plan, n_x[c], io_ratios[c]), a clip of more than 2^30 cotangent samples, in_abs0 /
 * out_k0 != 0, integer element types, HIPSOXR_F16 / HIPSOXR_BF16, any other selector (HIPSOXR_KERNEL_ADJOINT_AUTO, _FFT and
 * _TWO_STAGE included).  No clips, no channels or out_frames == 0: success, nothing launched.  Asynchronous on `hip_stream`. */
HIPSOXR_API hipsoxr_error_t hipsoxr_run_device_vr_ragged_adjoint(hipsoxr_plan_t *, const hipsoxr_job_t *job,
                                                                 const double *io_ratios /* host, n_clips */, void *hip_stream);

/* ---- stream: the soxr_t counterpart (host pointers, state carried across calls) ----------- */
HIPSOXR_API hipsoxr_error_t hipsoxr_stream_create(double in_rate, double out_rate,
                                                  unsigned num_channels,
                                                  hipsoxr_datatype_t io_type, /* itype == otype */
                                                  unsigned long recipe, unsigned long flags,
                                                  hipsoxr_stream_t **out);
/* Share an existing plan (no filter design); the plan must outlive the stream. */
HIPSOXR_API hipsoxr_error_t hipsoxr_stream_create_with_plan(hipsoxr_plan_t *, unsigned num_channels,
                                                            hipsoxr_datatype_t io_type,
                                                            unsigned long flags,
                                                            hipsoxr_stream_t **out);
/* soxr_process semantics: `in` = T const* (interleaved) or T const* const* (split); in == NULL
 * marks end of input (flush; call until *odone == 0); ilen == 0 with in != NULL drains only.
 * All of `ilen` is always consumed.  At most `olen` frames are written; *odone = frames written. */
HIPSOXR_API hipsoxr_error_t hipsoxr_stream_process(hipsoxr_stream_t *, const void *in, size_t ilen,
                                                   void *out, size_t olen, size_t *odone);
/* The same call on DEVICE buffers (round 4; version 0.4.1; round 5: small constant-rate calls are ONE dispatch — the kernel appends the chunk): `in` / `out` are device pointers (interleaved streams only),
 * the chunk is appended to the stream's ring by a device-to-device copy and every output the input so far determines is
 * written straight into `out`, all enqueued on `hip_stream` (a hipStream_t; NULL = default stream) — asynchronous, no
 * copy over PCIe, no host synchronisation; *odone is known at once (it is a function of the counts alone).  The caller
 * keeps `in` valid until the copy has run and orders its own use of `out` on `hip_stream`.  Same contract otherwise
 * (in == NULL: end of input; variable-rate streams and hipsoxr_stream_set_io_ratio included); frames and call
 * boundaries are those of hipsoxr_stream_process on the same input.  What CSoxr::process (src/soxr_ext.cpp:129-187)
 * would be for a caller whose audio already lives in HBM.  Not for streams created with HIPSOXR_DEFER / HIPSOXR_RESIDENT
 * flags or the split layout.  A stream created with HIPSOXR_STREAM_FFT (version 0.7.0) emits the same frame counts through the
 * frequency-domain engine. */
HIPSOXR_API hipsoxr_error_t hipsoxr_stream_process_device(hipsoxr_stream_t *, const void *in, size_t ilen,
                                                          void *out, size_t olen, size_t *odone, void *hip_stream);
/* Many INDEPENDENT streams in one call (round 5; version 0.5.0): handles[i] gets chunk ins[i] / ilens[i] and writes up to
 * olens[i] frames to outs[i], exactly as n calls of hipsoxr_stream_process_device in index order would — same frames,
 * same counters, bit for bit — but streams that share a plan (rates, quality), element type, channel count and device are
 * served by ONE kernel launch on `hip_stream`, whatever their phases and pending counts (a service with N live callers
 * at 10 ms chunks: one dispatch per tick instead of 2 N).  Streams the shared launch does not take (variable rate, end
 * of input, 4096 or more outputs due, mixed plans) are processed one by one inside the same call.  What N threads around
 * CSoxr::process (reference src/soxr_ext.cpp:129-187, tests/bench.py:71-88) would be for callers whose audio lives in HBM. */
HIPSOXR_API hipsoxr_error_t hipsoxr_streams_process_device(hipsoxr_stream_t *const *handles, size_t n, const void *const *ins,
                                                           const size_t *ilens, void *const *outs, const size_t *olens,
                                                           size_t *odones, void *hip_stream);
HIPSOXR_API void hipsoxr_stream_delete(hipsoxr_stream_t *);
HIPSOXR_API hipsoxr_error_t hipsoxr_stream_clear(hipsoxr_stream_t *);
HIPSOXR_API double hipsoxr_stream_delay(hipsoxr_stream_t *);
HIPSOXR_API size_t hipsoxr_stream_num_clips(hipsoxr_stream_t *);
HIPSOXR_API const char *hipsoxr_stream_engine(hipsoxr_stream_t *);
HIPSOXR_API hipsoxr_error_t hipsoxr_stream_set_io_ratio(hipsoxr_stream_t *, double io_ratio,
                                                        size_t slew_len);
HIPSOXR_API hipsoxr_plan_t *hipsoxr_stream_plan(hipsoxr_stream_t *);
/* int16 output is TPDF-dithered with a counter-based hash of (seed, channel, absolute output index):
 * deterministic and chunk-invariant.  libsoxr seeds its dither randomly per handle (the reference xfails
 * exact equality of int16 results for that reason, tests/test_resample.py:208-211); here the seed is 0
 * unless set, so equal inputs give equal outputs — and two streams with the same seed dither alike.
 * Give concurrent streams distinct seeds to decorrelate them. */
HIPSOXR_API hipsoxr_error_t hipsoxr_stream_set_dither_seed(hipsoxr_stream_t *, uint32_t seed);

/* ---- one-shot (create + process all + flush + delete), host pointers ---------------------- */
HIPSOXR_API hipsoxr_error_t hipsoxr_oneshot(double in_rate, double out_rate, unsigned num_channels,
                                            const void *in, size_t ilen, void *out, size_t olen,
                                            size_t *odone, hipsoxr_datatype_t io_type,
                                            unsigned long recipe, unsigned long flags);

#ifdef __cplusplus
}
#endif
#endif /* HIPSOXR_H */
