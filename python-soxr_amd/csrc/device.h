// device.h — interface between the host engine (engine.cpp) and the HIP side (kernels.hip).
#pragma once
#include "../../include/hipsoxr.h"
#include "plan.h"
#include "stream_rules.h" // VrPos

namespace hipsoxr {

// Build (once per precision) the device tables of a plan.  prec: 0 = f32 engine, 1 = f64 engine.
const char *device_bank_ensure(Plan *p, int prec);
void device_bank_release(Plan *p);

// Engine precision used for an element type: f32 for f32/i16/f16/bf16, f64 for f64/i32.
inline bool elem_is_half(int elem) { return elem == HIPSOXR_F16 || elem == HIPSOXR_BF16; }
inline int engine_prec(int elem) { return (elem == HIPSOXR_F32 || elem == HIPSOXR_I16 || elem_is_half(elem)) ? 0 : 1; }
inline size_t elem_size(int elem)
{
    return elem == HIPSOXR_F32 ? 4 : elem == HIPSOXR_F64 ? 8 : elem == HIPSOXR_I32 ? 4 : 2;
}

// Resident form of the small-launch kernel (kernels.hip, k_chain_resident): the mailbox in pinned host memory
// and what a launch of an instance needs.
static constexpr unsigned kResidentMaxWgs = 64;
// Watchdog: whatever HIPSOXR_RESIDENT_IDLE_US says, an instance that has heard nothing for this long leaves — a kernel that
// spins holds every device-wide synchronisation of the process (torch.cuda.synchronize() included) until it does.
static constexpr int kResidentWatchdogUs = 20000;
struct ResidentBox {
    uint64_t w[16];                 // lines 0-1: host -> device (tagged words, see k_chain_resident): 5 of them for a constant-rate
                                    // message, 14 with a variable-rate clock (three 128-bit numbers in 48-bit pieces); w[15] = leave
    uint32_t exited, pad[15];       // line 1: device -> host: the instance that has left
    uint32_t done[kResidentMaxWgs]; // lines 2..5: device -> host: last message finished, per workgroup
};
struct ResidentCtl { unsigned long long dec; unsigned arrived, pad; };
struct ResidentLaunch {
    ResidentBox *box;      // pinned, device-mapped
    const uint64_t *words; // where the instance reads the host -> device words: box->w, or 64 bytes of device memory
                           // the CPU stores into directly (large-BAR systems: a shorter trip, see engine.cpp)
    ResidentCtl *ctl;      // device memory, zeroed, not used by an earlier instance
    uint32_t base_seq;     // messages taken by earlier instances
    uint32_t epoch;        // number of this instance (never 0)
    int64_t idle_us;       // the instance leaves after this long without a message
    int64_t used_mcu = 0;  // in: milli-CUs already held by this process's resident instances
    int budget_shift = 1;  // in: resident instances may hold (CUs >> budget_shift) of the chip together
    uint32_t n_wgs = 0;    // out: workgroups of the instance
    int64_t max_out = 0;   // out: outputs per column one message may ask for
    uint32_t cost_mcu = 0; // out: CU capacity the instance occupies, n_wgs * 1024 / (workgroups that fit one CU)
    bool over_budget = false; // out: refused because used_mcu + cost_mcu would exceed the budget
};
// Completion words for a small launch: if the job turns out to be ONE launch of the small-launch kernel (k_chain) of at
// most `cap` workgroups, each workgroup stores `seq` into words[w] (pinned host memory) after its results are in host
// memory, and n_wgs says how many words to wait for; otherwise n_wgs = 0 and the caller waits for the stream.
// Polling these costs nothing; an event costs a record call, the command processor's signal after the kernel has
// drained, and the query calls (~4 us per streaming call).
struct ChainDone { uint32_t *words; uint32_t cap, seq; uint32_t n_wgs = 0; };
// Enqueue one job (validated by the caller) on `stream`.  vr != nullptr: positions come from *vr
// instead of the plan's rational ratio (interpolated-phase plans only).
// res: job.out_frames = the largest message the instance must serve; launches nothing but the resident kernel
const char *launch_job(Plan *p, const hipsoxr_job_t &job, void *stream, const VrPos *vr = nullptr, ResidentLaunch *res = nullptr,
                       ChainDone *cd = nullptr);
// hand message `seq` to the instance: outputs [out_k0, out_k0 + out_frames) from ring frames [in_abs0, in_abs0 + in_frames)
bool resident_post(const Plan &p, volatile uint64_t *words, uint32_t seq, int64_t in_abs0, int64_t in_frames, int64_t out_k0, int64_t out_frames,
                   const VrPos *vr = nullptr);
void resident_leave(volatile uint64_t *words, uint32_t epoch);

int device_count();
// what every entry that needs a device answers without one
constexpr const char *kNoDevice = "no HIP device available (hipsoxr has no CPU fallback)";

// Dynamic LDS above 64 KB needs hipFuncAttributeMaxDynamicSharedMemorySize raised on the function: a driver call, made
// once per (function, device) and high-water mark of the sizes asked for — not inside every launch.
const char *ensure_dyn_lds(const void *fn, size_t bytes);

// Environment switches, read ONCE per process.  The product library reads four names:
//   HIPSOXR_NO_FFT, HIPSOXR_RESIDENT, HIPSOXR_AUTO_RESIDENT, HIPSOXR_RESIDENT_IDLE_US.
// Everything else is an A/B or timing-experiment switch behind the numbers in DESIGN.md / profiles/ and is compiled in
// only with -DHIPSOXR_DEBUG_SWITCHES (build.sh makes that build beside the product: _variants/dbg/libhipsoxr.so, loaded
// through HIPSOXR_LIBRARY by tests/test_gpu_switches.py, tests/test_gpu_launch_forms.py and tools/*.sh).  None of them
// changes results beyond what the selected engine implies (dbg_flags excepted: timing only).
struct Switches {
    // ---- product ----
    bool no_fft = false;          // HIPSOXR_NO_FFT           AUTO never picks the frequency-domain engine (every job bit-exact)
    bool resident = false;        // HIPSOXR_RESIDENT         small-chunk synchronous streams use the resident kernel (as the HIPSOXR_RESIDENT flag)
    bool auto_resident = false;   // HIPSOXR_AUTO_RESIDENT    streams turn the resident path on by themselves after 16 small back-to-back calls
    int resident_idle_us = 1000;  // HIPSOXR_RESIDENT_IDLE_US an idle resident kernel leaves after this long (at most kResidentWatchdogUs = 20 ms)
    // ---- debug builds only (-DHIPSOXR_DEBUG_SWITCHES) ----
    bool fft_no_pair = false;     // HIPSOXR_FFT_NO_PAIR      one block per workgroup instead of the paired kernels
    bool fft_no_chpair = false;   // HIPSOXR_FFT_NO_CHPAIR    pair blocks even for interleaved even-channel data
    bool fft_no_xcd_map = false;  // HIPSOXR_FFT_NO_XCD_MAP   plain (block, column) workgroup ids for interleaved data
    bool fft_large_only = false;  // HIPSOXR_FFT_LARGE_ONLY   never the small-block variant
    bool fft_small_only = false;  // HIPSOXR_FFT_SMALL_ONLY   always the small-block variant
    bool fft_no_tiny = false;     // HIPSOXR_FFT_NO_TINY      never the quarter-size blocks
    int dbg_fft_k = 0;            // HIPSOXR_DEBUG_FFT_K      one-round float32 jobs (fft.hip, kOneRoundCost): k > 0 forces blocks of k periods, k < 0 = the size thresholds alone
    bool fft_no_wave = false;     // HIPSOXR_FFT_NO_WAVE      never the one-wave-per-pair kernel (fftwave.hip)
    int dbg_wave_min = 0;         // HIPSOXR_DEBUG_WAVE_MIN   ... from this many block pairs up (default 4096)
    int dbg_wave_slots = 0;       // HIPSOXR_DEBUG_WAVE_SLOTS ... at most this many persistent waves per launch (default: what the chip holds)
    bool no_planes = false;       // HIPSOXR_NO_PLANES        k_tile_mfma instead of k_tile_mfma_p
    bool no_mfma64 = false;       // HIPSOXR_NO_MFMA64        float64 engine (float64 / int32 I/O) on the vector ALU (k_tile) instead of v_mfma_f64
    bool no_host_ring = false;    // HIPSOXR_NO_HOST_RING     small-chunk streams keep their ring in device memory (copy per call)
    bool no_chain = false;        // HIPSOXR_NO_CHAIN         small launches on k_gather / k_interp
    bool no_done_words = false;   // HIPSOXR_NO_DONE_WORDS    streaming calls wait on an event, not on the kernel's completion words
    int direct_max = 0;           // HIPSOXR_DEBUG_DIRECT_MAX  largest result (bytes) a kernel writes straight into pinned host memory (0: engine.cpp's rule)
    bool resident_no_bar = false; // HIPSOXR_RESIDENT_NO_BAR  mailbox words and input stay in pinned host memory even on large-BAR systems
    bool no_xcd_split = false;    // HIPSOXR_NO_XCD_SPLIT     k_tile_mfma_p unit split on grid.z instead of XCD-aware ids
    bool no_tile_split = false;   // HIPSOXR_NO_TILE_SPLIT    k_tile / k_tile_mfma: never spread a slab's row tiles over several workgroups
    bool no_interp_tile = false;  // HIPSOXR_NO_INTERP_TILE   large interpolated launches on k_interp
    bool no_interp_wave = false;  // HIPSOXR_NO_INTERP_WAVE   mid-size interpolated / variable-rate launches on lane-per-output k_interp
    bool no_gather_wave = false;  // HIPSOXR_NO_GATHER_WAVE   exact-bank jobs below the tile kernels' size on k_chain / k_gather / the tile kernels as before
    int dbg_gw_taps = 0;          // HIPSOXR_DEBUG_GW_TAPS    k_gather_wave takes AUTO jobs of up to this many million output x tap products (default 16)
    bool no_two_stage = false;    // HIPSOXR_NO_TWO_STAGE     float device jobs of interpolated-phase plans stay on the exact engine
    // timing experiments on the tile kernels (results may be wrong with dbg_flags != 0)
    int dbg_flags = 0;            // HIPSOXR_DEBUG_FLAGS      1 no staging, 2 no LDS reads, 4 no coefficient loads, 8 no stores
    int dbg_nrt = 0, dbg_nw = 0;  // HIPSOXR_DEBUG_NRT / _NW  tiles / waves per workgroup
    int dbg_split = 0;            // HIPSOXR_DEBUG_SPLIT      grid.z unit split
    int dbg_chain_no = 0;         // HIPSOXR_DEBUG_CHAIN_NO   outputs per workgroup of k_chain (power of two <= 32)
    size_t dbg_lds = 0;           // HIPSOXR_DEBUG_LDS        extra dynamic LDS (occupancy experiments)
    bool dbg_slab32 = false;       // HIPSOXR_DEBUG_SLAB32     k_tile_mfma_p: 32-period slabs whatever the job size (A/B)
    bool no_halves = false;        // HIPSOXR_DEBUG_NO_HALVES  k_tile_mfma: both half-chains of a row tile on one wave for small jobs too (A/B)
    bool dbg_pad = false;          // HIPSOXR_DEBUG_PAD        k_tile_mfma: padded slab rows for odd periods too (round 2; A/B; read when a plan's tables are built)
    bool dbg_slab64 = false;       // HIPSOXR_DEBUG_SLAB64     k_tile_mfma_p: 64-period slabs for small jobs too (round-2 behaviour; A/B)
    int dbg_mfma64_pb = 0;         // HIPSOXR_DEBUG_MFMA64_PB  k_tile_mfma64_p: periods per slab, 16 or 32 (default: 16 below 1536 slabs of 32)
    bool dbg_mfma64_split = false; // HIPSOXR_DEBUG_MFMA64_SPLIT k_tile_mfma64_p: units of 16 periods even where 4 divides the tile count
    size_t dbg_mfma64_lds = 0;    // HIPSOXR_DEBUG_MFMA64_LDS LDS budget (bytes) that picks the float64 MFMA kernel's slab: 64, 32 or 16 periods
    size_t dbg_fft_lds = 0;       // HIPSOXR_DEBUG_FFT_LDS    the same for the frequency-domain kernels
    int dbg_poly_r = 0;           // HIPSOXR_DEBUG_POLY_R     k_poly: force the outputs per thread and tile
    int dbg_poly_mid_budget = 0;  // HIPSOXR_DEBUG_POLY_MID_BUDGET  a clip table on the two-stage form: bytes of intermediate per range of columns (default kPolyMidBudget, 1 GiB) — forces the range cut on small tables (tests; same bits)
    bool no_interp_pair = false;  // HIPSOXR_NO_INTERP_PAIR   k_interp_tile: one output per lane (A/B)
    bool dbg_interp_no_twin = false;     // HIPSOXR_DEBUG_INTERP_NO_TWIN      ... float pairs on ONE copy of the staged span (8-byte reads) always (A/B, tests)
    bool dbg_interp_pair_always = false; // HIPSOXR_DEBUG_INTERP_PAIR_ALWAYS  ... two per lane wherever a pair exists, whatever the cost model says (tests)
    bool adj_interp_per_lane = false; // HIPSOXR_DEBUG_ADJ_INTERP_PER_LANE  k_adj_interp: every lane walks its own k range instead of the wave's union (A/B; same bits)
    bool poly_no_pair = false;    // HIPSOXR_POLY_NO_PAIR     interleaved channel pairs on k_poly (one channel per pass) instead of k_poly2 (A/B)
    int dbg_tile_form = 0;        // HIPSOXR_DEBUG_TILE_FORM  k_tile_mfma_p: force launch form 1..4 (slab 64 whole / 64 split / 32 whole / 32 split)
    const char *dbg_trace = nullptr; // HIPSOXR_DEBUG_TRACE   path for per-wave s_memtime stamps (k_tile_mfma_p; k_fft_pair2 with -DFFT2_TRACE)
    const char *dbg_launch_log = nullptr; // HIPSOXR_DEBUG_LAUNCH_LOG  path of a text file: launch_fft_impl (fft.hip) appends one line per call — form, table row, instance kind, launch shape (written by the launcher of the form that took the job, or "none" by the dispatcher); adj_launch (adjoint.hip) one line per launch — kernel, element width, lanes, LDS bytes, channel group, launch shape (a ragged launch appends ragged=<n_clips>); launch_tile and launch_ragged (kernels.hip, tile_launch_log) one line per tile launch of the exact engine — kernel tile | tile_mfma | tile_mfma_p | tile_mfma64_p (a ragged launch also: gather), element width, io type, L M Lc Mc, pb, n_rt, nw (waves that compute), split (workgroups per slab), halves, xz, LDS bytes, launch shape; a ragged launch appends ragged=<n_clips> (equal-length launches of launch_gather's family: below); adj_interp_launch: kernel, element width, L M T P, tile frames, chunk size, LDS bytes, walk, launch shape; launch_poly (twostage.hip) one line per polyphase launch of the two-stage form — kernel poly | poly2, element width, taps, MQ, il (channel pairs), split, R, lane multiplier and its conflict cost, LDS bytes, channel group, columns, tiles, launch shape, outputs of member 1 and member 2 (a launch over a clip table's columns appends ragged=<columns>, tiles and n_out then being the longest column's — as does the FFT line of a launch over a table); launch_gather (kernels.hip) one line per launch — kernel gather_wave | chain | chain_resident | interp_wave | interp_tile | interp | gather, element width, io type, vr, L M T P, done nf cols, k0 in_abs0 (the launch's first output and the absolute index of input frame 0), launch shape, LDS bytes, then the form's own fields (chain: NO span_cap mode; wave forms: span_cap; tile: KO pair twin h nf_t m2_n span_cap; lane per output: ch_fast)
};
const Switches &switches();
// (engine.cpp) what the debug-switch build exports as hipsoxr_debug_stream_seek — no header declares it, the product does not
// export it: a fresh stream's counters set to (in_frames, out_frames), for tests of the stream kernels at large positions
const char *debug_stream_seek(hipsoxr_stream_t *s, uint64_t in_frames, uint64_t out_frames);

// One independent stream's part of a many-streams launch (kernels.hip k_chain_multi; engine.cpp
// hipsoxr_streams_process_device): the small-launch kernel's job description per stream, plus the chunk this call appends
// to the stream's ring — frames the launch reads straight from the caller's buffer while its workgroups copy them into the
// ring for the calls to come (one dispatch per call instead of a copy kernel and a launch).
struct ChainItem {
    const void *ring;    // the stream's device ring: frame 0 of it is absolute input frame in_abs0
    const void *chunk;   // this call's new frames (device memory, the stream's own layout), or nullptr
    void *out;           // where this stream's outputs go
    void *clip_counter;  // device counter of saturated integer outputs (or nullptr)
    int64_t in_abs0;     // absolute index of ring frame 0
    int64_t in_frames;   // ring frames that count for this launch, INCLUDING the chunk's
    int64_t split;       // first ring-relative frame that (still) lives in `chunk` (= in_frames - chunk_frames)
    int64_t chunk_frames;
    int64_t out_k0, out_frames; // outputs [out_k0, out_k0 + out_frames)
    int64_t d0, p0;      // out_k0 * M = L * d0 + p0 (exact-bank plans)
    uint32_t dither_seed, pad;
    // Ring compaction rides on the same launch: when ring_dst != ring the workgroups copy the frames still needed —
    // ring frames [keep_from, split) — to the start of ring_dst and the chunk behind them; the NEXT launch's ring is ring_dst
    // (frame 0 of it = absolute frame in_abs0 + keep_from).  ring_dst == ring: the chunk goes to ring frame `split`.
    void *ring_dst;
    int64_t keep_from;
    int64_t reserved;    // (sizeof = 128: the table is staged 16 bytes per thread)
};
// n_items streams of one plan, element type and channel count in ONE launch of the small-launch kernel (constant rate;
// every stream < 4096 outputs).  items_dev: the same table where the device can read it (pinned, device-mapped host
// memory is fine) — not needed for one item, which travels in the kernel arguments.  *handled = false: not a job for
// this kernel, nothing was launched.
const char *launch_chain_items(Plan *p, int elem, uint32_t n_channels, bool dither, const ChainItem *items, const ChainItem *items_dev,
                               uint32_t n_items, void *stream, bool *handled);

// device-to-device copy as an ordinary kernel launch on `stream` (a stream's chunk appended to its ring: hipMemcpyAsync costs
// ~2x the API time and queues behind a barrier packet)
const char *launch_copy(void *dst, const void *src, size_t bytes, void *stream);

// frequency-domain engine (fft.hip): whole-signal float32 / float64 jobs; int16 / int32 jobs that name it
// (HIPSOXR_KERNEL_FFT_PCM); float16 / bfloat16 jobs where a fused form exists (unit-stride columns, channel pairs: *handled
// stays false otherwise and launch_job_half runs half.hip's passes).  ch0: index of the job's channel 0 in the caller's whole
// signal (the dither key of jobs folded over channel ranges)
bool fft_job_eligible(const Plan &p, const hipsoxr_job_t &job);
const char *launch_fft(Plan *p, const hipsoxr_job_t &job, void *stream, bool *handled, uint32_t ch0 = 0);
// Streams on that engine (HIPSOXR_STREAM_FFT, engine.cpp): fft_stream_refusal names what it cannot serve (nullptr: served)
// and reports the periods of input a block reads in front of its first kept output; launch_fft_window is the chunk's job —
// outputs [job.out_k0, out_k0 + out_frames) of a column whose samples [in_abs0, in_abs0 + in_frames) are at job.in, zero
// outside — on the paired kernels only (*handled = false: not served, nothing launched; the caller's error).
const char *fft_stream_refusal(const Plan &p, int elem, uint32_t n_channels, int32_t *lead_periods);
const char *launch_fft_window(Plan *p, const hipsoxr_job_t &job, void *stream, bool *handled, uint32_t ch0 = 0);
void fft_release(const Plan *p);
// two-stage form for interpolated-phase plans (twostage.hip): FFT stage at 1:2 / 2:1 + a short polyphase stage in LDS
const char *launch_two_stage(Plan *p, const hipsoxr_job_t &job, void *stream, bool *handled);
// ... on a clip table (job.clip_table, validated by launch_job_table; float32 / float64, HIPSOXR_KERNEL_AUTO, any positive frame stride):
// a constant number of launches — per range of columns one ragged polyphase launch and one ragged FFT-stage launch, plus
// one launch_ragged_short for the clips the two-stage form does not admit.  *handled = false: not a table this path serves,
// or the FFT stage declined — the caller's clip-by-clip loop computes every clip.
const char *launch_two_stage_ragged(Plan *p, const hipsoxr_job_t &job, void *stream, bool *handled);
// (kernels.hip) the short clips of such a table — job.clip_table / clip_table_dev: the compacted sub-table — in one ragged
// launch of the exact engine's interpolated kernels, the engine and the bits of each clip alone; *handled as launch_ragged_job's
const char *launch_ragged_short(Plan *p, const hipsoxr_job_t &job, void *stream, bool *handled);
// (kernels.hip) the device copy of a job's clip table: job.clip_table_dev where the caller gave one (trusted to equal the
// host table), else the validated host table uploaded in stream order — *tmp is then what the caller releases with
// hipFreeAsync behind its launches.  texts: the caller's words for the two failures.
struct ClipTableTexts { const char *no_memory, *upload_failed; };
constexpr ClipTableTexts kRaggedTableTexts = {"ragged batches: no device memory for the clip table", "ragged batches: clip table upload failed"};
const char *clip_table_device(const hipsoxr_job_t &job, void *stream, const int64_t **rows, void **tmp, const ClipTableTexts &texts = kRaggedTableTexts);
// (kernels.hip) hipsoxr_run_device_vr_ragged's launch: job.clip_table validated by the entry, clock = the n_clips steps
// {hi, lo} of its io ratios (host memory; vr_ragged_rules.h) — one launch of a VR && RAGGED kernel per range of clips
const char *launch_vr_ragged(Plan *p, const hipsoxr_job_t &job, const uint64_t *clock, void *stream);
// transposed operator of the exact engine (adjoint.hip; hipsoxr_run_device_adjoint): job.in = gy (in_frames of it), job.out = gx
// (out_frames of it); validates the job itself.  HIPSOXR_KERNEL_ADJOINT: interpolated-phase plans too (k_adj_interp on the
// forward's own table, device_bank_ensure).  adjoint_release drops the plan's transposed tables (rebuilt on next use).
const char *launch_adjoint(Plan *p, const hipsoxr_job_t &job, void *stream);
const char *launch_adjoint_ragged(Plan *p, const hipsoxr_job_t &job, void *stream); // hipsoxr_run_device_adjoint_ragged: job.clip_table, one launch
// ... of a ragged variable-rate launch (hipsoxr_run_device_vr_ragged_adjoint): job.clip_table = rows {gy offset, n_y, gx offset,
// n_x} validated by the entry, clock = the n_clips steps {hi, lo} of its io ratios (host memory) — one launch of k_adj_interp<.., VR>
const char *launch_adjoint_vr_ragged(Plan *p, const hipsoxr_job_t &job, const uint64_t *clock, void *stream);
void adjoint_release(const Plan *p);
// ... on the frequency-domain engine (adjoint_fft.hip; HIPSOXR_KERNEL_ADJOINT_FFT, which the two entries above hand over
// first thing): the forward float job of the plan's transposed plan through launch_fft, or an error by name — never the
// exact adjoint.  adjoint_fft_release drops the transposed plan (adjoint_release calls it).
const char *launch_adjoint_fft(Plan *p, const hipsoxr_job_t &job, void *stream);
const char *launch_adjoint_fft_ragged(Plan *p, const hipsoxr_job_t &job, void *stream);
void adjoint_fft_release(const Plan *p);
// (adjoint_fft.hip) the transposed plan of an exact-bank plan as a fresh Plan the caller owns: L' = M, M' = L, the mirrored
// prototype (adjoint_fft_rules.h), the forward's recipe and device — what both fast adjoints hand to launch_fft
Plan *adj_fft_transposed(const Plan &p);
// ... of the two-stage form (twostage.hip; HIPSOXR_KERNEL_ADJOINT_TWO_STAGE, handed over by launch_adjoint first thing):
// interpolated-phase plans the forward two-stage form takes — the transposed plan of its FFT stage through launch_fft and
// k_poly_adj, or an error by name — never the exact adjoint
const char *launch_adjoint_two_stage(Plan *p, const hipsoxr_job_t &job, void *stream);
// ... and the transpose of the job HIPSOXR_KERNEL_AUTO launches (adjoint_auto.hip; HIPSOXR_KERNEL_ADJOINT_AUTO, handed over by both
// entries first thing): the frequency-domain engine, the transposed two-stage form — a clip table too — or the exact adjoint,
// by adjoint_auto_rules.h; never "unavailable".  It puts together the inner functions of the three launchers:
//   adj_fft_try (adjoint_fft.hip): the transposed plan's float job through launch_fft; *handled = false, nothing queued: declined
//   launch_adjoint_two_stage_try (twostage.hip): the equal-length transposed form behind its refusals; *handled as above
//   launch_adjoint_two_stage_ragged (twostage.hip): a validated clip table — per range k_poly_adj<.., RAGGED> and the FFT stage's
//     transposed plan, the short clips through adj_exact_run; *handled = false: gx untouched, the exact adjoint takes the table
//   adj_exact_run (adjoint.hip): the exact adjoint's tables and — unless dry — its launch; rows: a table's device copy, or NULL
const char *launch_adjoint_auto(Plan *p, const hipsoxr_job_t &job, void *stream);
const char *launch_adjoint_auto_ragged(Plan *p, const hipsoxr_job_t &job, void *stream);
const char *adj_fft_try(Plan *p, const hipsoxr_job_t &job, void *stream, const int64_t *rows, bool *handled);
const char *launch_adjoint_two_stage_try(Plan *p, const hipsoxr_job_t &job, void *stream, bool *handled);
const char *launch_adjoint_two_stage_ragged(Plan *p, const hipsoxr_job_t &job, void *stream, bool *handled);
const char *adj_exact_run(Plan *p, const hipsoxr_job_t &job, void *stream, const int64_t *rows, bool dry);
// float16 / bfloat16 jobs that no fused kernel takes (half.hip): one widening pass into stream-ordered float32 temporaries
// packed in the caller's dimension order, the float32 job of the same selector (adjoint: through launch_adjoint, else
// launch_job), one narrowing pass over exactly the job's output elements.  No clip_table (launch_table_clips, the clip-by-clip loop,
// re-enters with each clip as a plain job).
const char *launch_half(Plan *p, const hipsoxr_job_t &job, void *stream, bool adjoint);

} // namespace hipsoxr
