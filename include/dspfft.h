/*
 * dspfft.h -- device-resident C ABI of the MI355X real-even DCT engine.
 *
 * This is the second-level boundary of SURVEY.md section 8(b): the same plan/execute contract the
 * reference reaches through `fftw(call)` (include/precision.h:115 of the reference), but on DEVICE
 * pointers and an explicit HIP stream, so buffers stay resident in HBM between transforms.
 * include/fftw3.h (the FFTW-named host-pointer shim the tools link against) is a thin adapter over
 * these entry points.
 *
 * All functions return 0 on success and a negative code on failure; dspfft_last_error() describes
 * the most recent failure of the calling thread.  No function touches user arrays at plan time
 * (scan/scan.c:354-359 relies on that, see SURVEY.md section 7 "FFTW_MEASURE clobbering").
 */
#ifndef DSPFFT_H
#define DSPFFT_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* same numeric values as FFTW's fftw_r2r_kind for the two kinds the reference uses */
enum { DSPFFT_REDFT01 = 4, DSPFFT_REDFT10 = 5 };

typedef struct dspfft_plan_s *dspfft_plan;

/* Replaces fftw(plan_many_r2r) -- spec/spec.c:63, spec/ispec.c:165, zoom/zoom.c:263, scan/scan.c:292,359,
 * motion/motion.c:535-538,549-552.  rank 1..3, kinds[i] in {DSPFFT_REDFT10, DSPFFT_REDFT01}, f32 data.
 * Addressing follows FFTW's advanced interface: element (i0..i_{r-1}) of transform t is at
 * t*dist + stride*(((i0*embed[1] + i1)*embed[2] + i2)); embed == NULL means embed = n. */
int dspfft_plan_many_r2r(dspfft_plan *plan, int rank, const int *n, int howmany,
                         const int *inembed, int istride, int idist,
                         const int *onembed, int ostride, int odist, const int *kinds);

/* Replaces fftw(plan_r2r_2d) -- applybasis/draw.c:74. */
int dspfft_plan_r2r_2d(dspfft_plan *plan, int n0, int n1, int kind0, int kind1);

/* Fused per-index normalisation: every output is multiplied by `scale`; along
 * transformed axis `axis` (0-based, as in n[]) input index 0 is multiplied by in_scale0 before the
 * transform and output index 0 by out_scale0 after it.  Defaults: 1, 1, 1.
 *   spec/spec.c:70-78     = scale 1/(2wh), out_scale0 1/sqrt2 on both axes
 *   spec/ispec.c:153-159  = scale 1/2,     in_scale0  sqrt2   on both axes
 *   scan/scan.c:296-298   = scale 1/(4wh)
 *   motion/motion.c:644-647 (block == scaled) = scale 2 sqrt2, out_scale0 1/sqrt2 on all three axes */
int dspfft_plan_set_scale(dspfft_plan plan, float scale);
int dspfft_plan_set_axis_scale0(dspfft_plan plan, int axis, float in_scale0, float out_scale0);

/* Replaces fftw(execute) -- 9 call sites.  d_in/d_out are DEVICE pointers laid out as
 * the plan describes; d_in == d_out is the in-place case.  Asynchronous on `hip_stream`
 * (a hipStream_t; NULL = the default stream). */
int dspfft_execute(dspfft_plan plan, const float *d_in, float *d_out, void *hip_stream);

/* Profiling aid: a plan is a sequence of 1-D axis passes (one kernel launch each, last axis
 * first).  dspfft_execute_pass runs pass `index` alone, exactly as dspfft_execute would (pass 0
 * reads d_in, later passes work in place on d_out), so each kernel can be bracketed by events. */
int dspfft_plan_num_passes(dspfft_plan plan);
int dspfft_execute_pass(dspfft_plan plan, int index, const float *d_in, float *d_out, void *hip_stream);

/* Many executions with one call: item i runs plans[i] on (d_in[i], d_out[i]) on hip_streams[i] (f32 plans), in order.  This is what
 * a tool that loops fftw(execute) over the frames of a clip (motion/motion.c:613-753, scan/scan.c:447) calls once per batch, so a
 * binding layer (cgo, ctypes ...) pays its per-call cost once per batch instead of once per frame and pass.
 * Profiling aid: with pass_events non-NULL, every pass of items [timed_item, timed_item + timed_count) is bracketed by events
 * recorded on that item's stream: the j-th bracketed pass between pass_events[2j] and pass_events[2j+1] (handles from
 * dspfft_event_create; read with dspfft_event_elapsed_ms after dspfft_event_synchronize or a stream/device synchronise). */
int dspfft_execute_many(int count, const dspfft_plan *plans, const float *const *d_in, float *const *d_out, void *const *hip_streams,
                        int timed_item, int timed_count, void *const *pass_events);
/* The same batch `repeats` times with ONE call: the frame loop of a clip inside the library (motion/motion.c:613-753 executes its
 * per-frame plans once per frame, scan/scan.c:421-447 its inverse plan once per output frame), so nothing of the host language sits
 * between two frames.  rejoin_every > 0 and more than one distinct stream in the batch: every rejoin_every repeats each stream waits
 * for the point the others have reached (two free-running streams otherwise keep whatever relative phase the first repeat's host timing
 * gave them, and that phase decides how well their kernels share the CUs).
 * Profiling aid: with pass_events non-NULL and timed_every > 0, repeats 0, timed_every, 2 timed_every ... bracket every pass of a window
 * of timed_count consecutive items (timed_count must divide count); the window advances by timed_count items (mod count) each time, and
 * the events of the j-th bracketed pass overall are pass_events[2j], pass_events[2j+1].  One-pass block plans cannot be bracketed.
 * Items may be f32 or f64 plans: each item's buffers are float or double as its plan says (hence the void pointers). */
int dspfft_execute_many_repeat(int count, const dspfft_plan *plans, const void *const *d_in, void *const *d_out, void *const *hip_streams,
                               int repeats, int rejoin_every, int timed_every, int timed_count, void *const *pass_events);
/* Forward/inverse pairs.  Both calls above may run two adjacent items i, i + 1 as ONE roundtrip (what dspfft_execute_roundtrip runs without
 * a filter) when all of this holds: both plans are f32; hip_streams[i] == hip_streams[i + 1]; the second item works in place on the first
 * one's output, d_out[i] == d_in[i + 1] == d_out[i + 1] (the first item may be in place or not); neither item lies in a timed window of
 * that repeat (timed items always run pass by pass, two events per pass); plans[i] is REDFT10 and plans[i + 1] REDFT01 on every axis over
 * the same layout, and the forward plan's last pass and the inverse plan's first (dspfft_plan_many_r2r_ordered(..., 1)) are column passes
 * along the same axis with the same specialised kernel -- listed, or compiled at plan time -- over the same tiles, without a host loop,
 * input window, modulation or alternating sign, on 16-byte-aligned buffers.  Those two passes then run as one kernel that keeps each tile in
 * LDS between them: the spectrum after the forward plan's last pass is NEVER STORED (the buffer holds the forward plan's earlier passes'
 * output until the roundtrip's own last passes overwrite it), which nothing ordered on that stream can observe.  The results are
 * bit-identical to the two items run pass by pass.  Items are scanned left to right and belong to one pair at most ((fwd, inv, fwd) pairs
 * the first two); a pair that fails any condition runs as two items, never as an error.  DSPFFT_NO_FUSED_ROUNDTRIP=1 (read per call)
 * turns the pairing off.
 * dspfft_many_fused_pairs: how many pairs this process has run that way so far (atomic, never reset). */
unsigned long long dspfft_many_fused_pairs(void);
/* The fused column kernel copies the twiddle factors it reads (one entry per stage twiddle, then T[k], k <= N/2; 8 bytes each) into the
 * LDS behind its tile where that costs no resident workgroup.  For the listed kernel of N rows x K floats on T threads: the bytes it
 * stages, 0 where it keeps loading them from global memory, -1 where no such kernel is listed.  A build-time property. */
long long dspfft_col_roundtrip_table_bytes(int N, int K, int T);
/* How many times this process has enqueued the fused column kernel so far, from any roundtrip entry or fused pair (atomic, never reset). */
unsigned long long dspfft_col_roundtrip_launches(void);
/* Streams of the library's own for the calls above: plain non-blocking HIP streams (hipStreamCreateWithFlags(hipStreamNonBlocking)),
 * for hosts without a HIP binding of their own (cgo, ctypes ...) and for hosts whose framework hands out streams from a pool:
 * two streams of torch's pool were seen sharing a hardware queue, which serialises the two frames they carry (48K instead of 56K
 * Mpix/s on the 4K roundtrip, tools/py_enqueue_probe.py).  NULL on failure. */
void *dspfft_stream_create(void);
void dspfft_stream_destroy(void *stream);
int dspfft_stream_synchronize(void *stream);
void *dspfft_event_create(void);
void dspfft_event_destroy(void *event);
int dspfft_event_synchronize(void *event);
int dspfft_event_elapsed_ms(void *start, void *stop, float *ms);

/* Double-precision samples: the fftw_ (no suffix) API that spec, zoom and applybasis use in their default
 * build (COEFF_PRECISION ?= D: spec/Makefile:1, applybasis/Makefile:1; include/precision.h:50-53,66-72).
 * Same geometry and call-site contract as above with `double` buffers; arithmetic, twiddle tables and the
 * fused scales are double.  These plans run the runtime-geometry kernels (the compile-time-specialised
 * ones are f32 only).  The _f64 scale setters also work on f32 plans (rounded to float there);
 * dspfft_execute on an f64 plan, or dspfft_execute_f64 on an f32 plan, fails with an error. */
int dspfft_plan_many_r2r_f64(dspfft_plan *plan, int rank, const int *n, int howmany,
                             const int *inembed, int istride, int idist,
                             const int *onembed, int ostride, int odist, const int *kinds);
int dspfft_plan_set_scale_f64(dspfft_plan plan, double scale);
int dspfft_plan_set_axis_scale0_f64(dspfft_plan plan, int axis, double in_scale0, double out_scale0);
int dspfft_execute_f64(dspfft_plan plan, const double *d_in, double *d_out, void *hip_stream);
/* Optional: the caller promises that input samples of `axis` outside [lo, hi) are ZERO (a spectrum zero-padded to a longer transform:
 * zoom's y stage, motion's scaled > block) so that they need not be read.  Returns 1 when the plan honours it -- then those rows need
 * not even be stored -- and 0 when it does not (nothing changes: the zeros must really be there).  Today: f32 plans whose first pass
 * is a listed specialised column or row REDFT01 pass along `axis`.  lo = hi = 0 turns it off.  Negative: bad arguments. */
int dspfft_plan_set_input_window(dspfft_plan plan, int axis, int lo, int hi);
/* On top of an input window (set it first; setting a window again drops this): input sample x of `axis` is taken from position
 * p = reversed_from > 0 ? reversed_from - x : x of its line and multiplied by d_mul[p] while it is loaded (d_mul: floats in device memory,
 * kept by the caller, indexed by position).  zoom's x stage reads ONE array twice this way -- T[u] cos(theta u) in its place and
 * T[M - x] sin(theta (M - x)) mirrored -- instead of having a kernel write both products out.  Returns 1 when honoured (f32 plans whose
 * first pass is a listed specialised row or column REDFT01 pass along `axis` with a window), 0 when not (nothing changes); d_mul = NULL: off. */
int dspfft_plan_set_input_modulation(dspfft_plan plan, int axis, const float *d_mul, int reversed_from);
/* Optional: output sample j of `axis` is multiplied by (-1)^j, fused into that axis's pass (with REDFT01 on index-reversed input this is
 * the sine counterpart of the transform: sum_u D[u] sin(pi (j + 1/2) u / M) = (-1)^j 1/2 REDFT01(E)[j], E[u'] = D[M - u'] -- the second
 * half of zoom's shifted cosine series).  Returns 1 when honoured (f32 plans whose pass along `axis` is a listed specialised column or row REDFT01
 * pass and the last of the plan), 0 when not (nothing changes).  Combined with dspfft_execute_masked_accumulate(plan, in, work, acc, NULL,
 * ...) the signed result is added into `acc` by the same pass. */
int dspfft_plan_set_output_alternate(dspfft_plan plan, int axis, int on);
/* d_out = a(d_in_a) + b(d_in_b): the sum of two plans' results, each with its own scale, input window and output sign.  ONE launch
 * that writes d_out once when both are f32 one-axis plans on the same listed row REDFT01 kernel over the same output lines (zoom's
 * x stage by fast transforms: cosine part + sine part); otherwise dspfft_execute(a) followed by an accumulating execution of b, for
 * which b must be a one-pass plan (-2 otherwise).  d_out must not overlap the inputs. */
int dspfft_execute_sum2(dspfft_plan a, dspfft_plan b, const float *d_in_a, const float *d_in_b, float *d_out, void *hip_stream);

/* ---- rows of a phase-shifted cosine series (zoom's x stage: zoom/zoom.c:361-368 with the basis of :36-68 on a DCT-III grid) ----
 *     out[j][b][c] = scale * sum'_{u < cw} in[j][u][c] cos(u (pi (b + 1/2) / M + theta)),    b < vw <= M, c < 3, j < lines
 * (sum' halves u = 0: zoom.c:364 `coeffs[..]/2`).  With theta = 0 this is 1/2 REDFT01_M of the zero-padded line; a non-zero theta is a
 * pan by theta M / pi samples (zoom.c:49-57 `offset`), which two transforms would need (cosine and sine part: dspfft_execute_sum2).
 * Here both parts ride through ONE half-length FFT per channel as the halves of a packed-FP32 pair: a kernel of its own
 * (dspfun_amd/csrc/dct_duo.h), three barrier-separated phases per channel, whole pixels stored once.
 * Scaled lengths M with a listed kernel only (spec_list.h DSPFFT_ZOOMX_SPECS: 7680, 5760, 3840, 2560, 1920, 1280): create returns -2 for the
 * others and the caller keeps dspfft_execute_sum2.  Lines: `in` cw pixels of 3 floats, in_pitch floats apart; `out` vw pixels, out_pitch
 * floats apart; 4-byte alignment suffices.  theta and scale are arguments of the execution (a pan re-plans nothing): the multiplier table
 * they determine (M/2 .. 2M slots of 16 bytes, evaluated in double on the device) is rebuilt per call, on the stream, in the plan's
 * own buffer -- one execution of a plan at a time. */
typedef struct dspfft_cosrows_s *dspfft_cosrows;
int dspfft_cosrows_create(dspfft_cosrows *plan, int M, int cw, int vw, int lines);
int dspfft_cosrows_execute(dspfft_cosrows plan, const float *d_in, long long in_pitch, float *d_out, long long out_pitch, double theta, double scale, void *hip_stream);
void dspfft_cosrows_destroy(dspfft_cosrows plan);

/* ---- rows of a cosine series at ANY sample spacing, by the chirp-z transform (zoom's product at scales off the DCT-III grid and for
 * the `centered` basis: zoom/zoom.c:36-68,361-375; dspfun_amd/csrc/dct_czt.h) ----
 *     out[b] = scale * sum'_{n < nc} in[n] cos(n (omega b + phi)),    b < nout           (sum' halves n = 0)
 * per line: a circular convolution of a listed smooth length P >= nc + nout - 1 (1200 ... 19200: spec_list.h DSPFFT_CZT_SPECS) in LDS,
 * forward FFT, times the chirp's spectrum, inverse FFT.  create returns -2 when nc + nout - 1 exceeds the longest listed P.
 * Lines come in `groups` of `group` members (1, or 3 = the channels of an image row, which share their output cache lines and are then run
 * on one XCD back to back): line (g, m) reads in[g * in_group + m * in_pitch + n * es_in] and writes out[g * out_group + m * out_pitch + b * es_out].
 * omega, phi and scale are arguments of the execution; the tables they determine live in the plan (one execution of a plan at a time);
 * the chirp's spectrum is rebuilt only when omega changes. */
typedef struct dspfft_cztrows_s *dspfft_cztrows;
int dspfft_cztrows_create(dspfft_cztrows *plan, int nc, int nout, int lines, int group);
int dspfft_cztrows_execute(dspfft_cztrows plan, const float *d_in, long long in_group, long long in_pitch, int es_in,
                           float *d_out, long long out_group, long long out_pitch, int es_out, double omega, double phi, double scale, void *hip_stream);
/* The same on a sub-extent: the first `lines` lines (a multiple of the group, <= the plan's lines), each of its first nc <= the plan's nc
 * components; samples past nc are never read (they may hold anything, NaN included).  dspfft_cztrows_execute is this call at the plan's
 * own extents.  The chirp's spectrum is made for the plan's nc and serves every smaller one. */
int dspfft_cztrows_execute_n(dspfft_cztrows plan, int nc, int lines, const float *d_in, long long in_group, long long in_pitch, int es_in,
                             float *d_out, long long out_group, long long out_pitch, int es_out, double omega, double phi, double scale, void *hip_stream);
int dspfft_cztrows_length(dspfft_cztrows plan);      /* the convolution length P the plan runs on */
void dspfft_cztrows_destroy(dspfft_cztrows plan);
/* out[c * out_pitch + r] = in[r * in_pitch + c], r < rows, c < cols (the re-layout between the two axes of a chirp-z zoom frame) */
int dspfft_transpose_f32(float *d_out, long long out_pitch, const float *d_in, long long in_pitch, int rows, int cols, void *hip_stream);
/* Optional, for owner ids that stay the same over the frames of a scan (every method but box, whose ids are stamped per frame):
 * records the (min, max) owner id of every column tile of `plan`, so that a later dspfft_execute_masked_accumulate with the SAME
 * d_ids pointer and elems_per_id leaves a tile alone -- without reading its owner ids -- when `id` lies outside its range.  Call it
 * again after rewriting the ids; d_ids = NULL forgets.  Results are the same with or without it.
 * For single-precision plans it also copies the ids into the order the column tiles read them, one element one id, one byte each (two when
 * some id is 255 or more; none when some id is 65535 or more): plan-owned device memory of 1 or 2 bytes per element of the image.  The
 * masked column pass of the step then reads that table instead of d_ids (8K RGB frame step 0.429 -> 0.379 ms); it synchronises
 * hip_stream once to look at the ranges.
 * The library cannot see writes to the id array: rewriting it (dspfft_scan_stamp, dspfft_scan_frame_ids, dspfft_scan_index_to_frame_ids
 * or your own kernel on the same buffer) WITHOUT preparing again makes later steps skip the wrong tiles.  The prepared ranges and the
 * per-tile flags are scratch of the plan: masked executions of one plan must be serialised on one stream (one plan per stream otherwise). */
int dspfft_plan_scan_prepare(dspfft_plan plan, const uint32_t *d_ids, int elems_per_id, void *hip_stream);
int dspfft_execute_masked_accumulate_f64(dspfft_plan plan, const double *d_in, double *d_work, double *d_acc,
                                         const uint32_t *d_ids, uint32_t id, int elems_per_id, void *hip_stream);

/* The shape of FFTW's guru interface (fftw_plan_guru_r2r; not called by the reference's tools, which loop over blocks
 * on the host instead: motion/motion.c:591-615): every transformed dimension and every batch dimension carries its own
 * extent and input / output strides (in elements).  One plan then covers, e.g., all 8x8x8 blocks of a [D][H][W] volume
 * (motion --blocksize 8x8x8, motion/README.md): dims = {8,HW,HW},{8,W,W},{8,1,1}, howmany_dims =
 * {D/8,8HW,8HW},{H/8,8W,8W},{W/8,8,8}.  rank 1..3, howmany_rank 0..6; f64 != 0 selects double samples.  Lengths up to
 * 32 run one line per thread in registers. */
typedef struct { int n; int is; int os; } dspfft_iodim;
/* Planning effort for the plans created after the call, on ANY thread of the process (plans already made keep theirs); a thread may override it for
 * the plans it makes itself with dspfft_set_thread_plan_effort (effort < 0 removes the override; dspfft_get_thread_plan_effort: -1 when none), which is
 * what the FFTW shim does around each fftw(plan_many_r2r).  dspfft_get_plan_effort returns the value in force for the calling thread.
 * 0 (default): a frame size without a compile-time-specialised kernel (spec_list.h) runs on the runtime-geometry kernels.
 * > 0: such sizes get RowSpecT / ColSpecT kernels COMPILED AT PLAN TIME (hiprtc: about a second per new size, then cached in
 * $DSPFFT_JIT_CACHE or ~/.cache/dspfft-jit) and run 1.3-1.8x faster from then on.
 * >= 2: several candidates (radix orders, thread counts, column tile widths) are compiled and TIMED on a scratch buffer, the fastest
 * is kept (the caller's arrays are never touched).  The FFTW shim maps FFTW_ESTIMATE to 0, FFTW_MEASURE (scan.c:359) to 1 and
 * FFTW_PATIENT / FFTW_EXHAUSTIVE (motion.c:93-103) to 2.  DSPFFT_JIT=1 / 2 in the environment forces compilation on / off,
 * DSPFFT_JIT_TUNE=1 / 2 the timed search. */
void dspfft_set_plan_effort(int effort);
int dspfft_get_plan_effort(void);
void dspfft_set_thread_plan_effort(int effort);
int dspfft_get_thread_plan_effort(void);
/* Diagnostic for the FFTW shim (include/fftw3.h): how many fftw(execute) calls of this process carried their input up as packed non-zero 4 KB blocks
 * instead of one dense copy.  Arrays of 32 MB and more are read by host threads first (DSPFFT_UPLOAD_THREADS, default = the CPU quota, at most 12;
 * 0 = never); an array more than a quarter non-zero goes up dense and is looked at again only after 1, 2, 4 ... 64 further executes.  What arrives on the
 * device is the same bytes either way (scan/scan.c:429-447: <= 3 % of `reconstruction` is set per output frame). */
unsigned long long dspfft_fftw_sparse_uploads(void);
int dspfft_plan_guru_r2r(dspfft_plan *plan, int rank, const dspfft_iodim *dims, int howmany_rank, const dspfft_iodim *howmany_dims,
                         const int *kinds, int f64);

/* As dspfft_plan_many_r2r, with the order of the axis passes chosen: first_axis_first = 0 is the default (last axis
 * first), 1 runs axis 0 first and the contiguous axis last.  The results are the same; the order decides which pass
 * reads the caller's input layout and which one ends the plan. */
int dspfft_plan_many_r2r_ordered(dspfft_plan *plan, int rank, const int *n, int howmany,
                                 const int *inembed, int istride, int idist,
                                 const int *onembed, int ostride, int odist, const int *kinds, int first_axis_first);
/* ... and dspfft_plan_guru_r2r (f32) with that choice */
int dspfft_plan_guru_r2r_ordered(dspfft_plan *plan, int rank, const dspfft_iodim *dims, int howmany_rank, const dspfft_iodim *howmany_dims,
                                 const int *kinds, int first_axis_first);

/* motion's transform -> filter -> inverse loop (motion/motion.c:641-753) as one call.  `fwd` is a REDFT10 plan in
 * the default order, `inv` a REDFT01 plan created with first_axis_first = 1, in place on fwd's output layout; then
 * fwd's last pass and inv's first pass run along the same axis, and when both have a specialised column kernel
 * they execute as ONE launch: the tile stays in LDS through forward transform, filter and inverse transform
 * (8 B/sample of HBM traffic instead of 24 for that axis and the filter).  Otherwise -- also when a plan carries
 * an input window, modulation or alternating output sign on that axis (dspfft_plan_set_*: the fused kernel and the 8-bit
 * row ends are plain instantiations) -- the three steps run separately.  filter == NULL skips the filter.  The filter is motion.c:683-744 (see dspfft_motion_filter below):
 * positions are taken inside blocks of block_depth planes of minbuf_hw[0] x minbuf_hw[1] elements (block_depth =
 * the embedding depth for one 3-D block, 1 when every frame is its own block, motion's default -b 0x0x1);
 * d_coeffs_coded (device, may be NULL) is incremented by the number of non-zero quantised coefficients.
 * Small blocks (motion --blocksize 8x8x8 and the like: every extent 4, 8 or 16, 2-D blocks up to 32; f32; x contiguous; planned
 * with dspfft_plan_many_r2r as a block-major stack or with dspfft_plan_guru_r2r where they lie in a volume): dspfft_execute runs all
 * axes of a block in ONE pass, and this call -- the _u8 form included -- runs load, forward transform, filter (positions are the
 * block's own coordinates), inverse transform and store as ONE kernel; the inverse plan needs no particular pass order then.
 * Buffers must be 16-byte aligned (8-bit ones: 4-byte) for that path; a filtered roundtrip over the blocks of a volume has no
 * other path and fails otherwise. */
typedef struct {
	int active[3];            /* block extent {d, h, w} actually transformed */
	int minbuf_hw[2];         /* rows and row pitch of the buffer's planes */
	int block_depth;
	int band_begin[3], band_end[3];
	float damp, boost, threshold_lo, threshold_hi;
	int preserve_dc;          /* 0 none, 1 dc, 2 grey */
	float grey_add, quantizer;
} dspfft_motion_filter_params;
int dspfft_execute_roundtrip(dspfft_plan fwd, dspfft_plan inv, const float *d_in, float *d_out,
                             const dspfft_motion_filter_params *filter, unsigned long long *d_coeffs_coded, void *hip_stream);

/* `scaled != block` (motion/motion.c:535-552,566,644-647,748-759): `inv` may be planned over DIFFERENT extents than `fwd` inside the
 * same embedding (same strides; howmany = 1).  Larger extents zero-pad the spectrum (band-limited upscale), smaller ones truncate
 * it (downscale); the filter's `active` is min(block, scaled) per axis.  The transforms then run unfused.  The work buffer is
 * zeroed first (motion.c:619) except in place on a float buffer, where the caller has zeroed everything outside the block.
 *
 * A whole GRID of such blocks (motion --blocksize 8x8x8 --size 4x4x4 over a clip, motion.c:488-499,613-800) is ONE launch of this call
 * and of its _u8, _u8_dither and _topn forms: every block is loaded, transformed over `block`, filtered over min(block, scaled),
 * transformed back over `scaled` and stored by one kernel (block_rescale.hip), the block's embedding never leaving the chip.  The pair is
 * such a grid when both plans are f32 small-block plans as described above (every extent of `block` and of `scaled` 4, 8 or 16, 2-D
 * blocks up to 32; x contiguous; strides multiples of 4), `fwd` REDFT10 and `inv` REDFT01 on every axis, of the same rank and axis order,
 * with the same numbers of blocks, and the extents differ.  Two layouts:
 *   volume layout      both dspfft_plan_guru_r2r, each in place on its OWN volume: `fwd` over the input [D][H][W] with dims `block` and
 *                      howmany {D/bd, H/bh, W/bw}; `inv` over the output [D sd/bd][H sh/bh][W sw/bw] with dims `scaled` and the same
 *                      howmany counts (strides of that volume)
 *   block-major layout both dspfft_plan_many_r2r with howmany = the number of blocks and idist = odist = the block's own volume
 *                      (bd bh bw for `fwd`, sd sh sw for `inv`)
 * d_in is read in `fwd`'s INPUT layout and d_out written in `inv`'s OUTPUT layout: the call is out of place by nature and the in-place
 * layout rules above do not apply to it.  Float buffers must be 16-byte aligned, 8-bit ones 4-byte.  The filter's `active` is the caller's
 * min(block, scaled); positions are the block's own coordinates (minbuf_hw and block_depth are not consulted).
 *   _u8         d_work is not touched and may be NULL (for every other pair it is required)
 *   _u8_dither  the kernel stores float into d_work in `inv`'s output layout (required here), and the dithered store writes the bytes over
 *               the output volume block by block -- the composition the block == scaled path uses
 *   dspfft_plan_set_u8_trc is honoured at both 8-bit ends, the dithered store included
 *   _topn       a keep in range is refused (-2, nothing launched): the reference selects over the whole embedding, forward coefficients
 *               outside min(block, scaled) included (motion.c:652-668), and these entries carry no factor to rank those with;
 *               keep == 0 or keep >= the embedding's count max(block, scaled) is the plain call
 *   _limit      the forms that take such a keep (dspfft_coeff_limit, below): one kernel of their own, block_rescale_topn.hip
 * -2, with the reason and nothing launched, also for misaligned buffers and for a pair that is almost a grid (different block counts, 2-D
 * against 3-D blocks, an extent outside the list); -3 from a library built without the HIP kernel.  A pair with block == scaled is the
 * path described above: the same kernels, the same bytes.
 *
 * Blocks ALONG TIME (motion --blocksize 1x1xD, with --size 1x1xD'; motion/README.md:87-89): every pixel of every run of D frames of a
 * [frames][H][W] plane is a 1-D block.  The pair is such a clip when both plans are f32 and rank 1, `fwd` REDFT10 of length D and `inv`
 * REDFT01 of length D', the transformed axis at stride P = H W > 1 in place, with a unit-stride batch dimension of exactly P samples and
 * at most one further batch dimension, the blocks, n P apart (n the plan's own length: `fwd` over the input clip, `inv` over the dense
 * output clip [blocks D'][H][W]), both plans counting the same blocks and pixels (dspfft_plan_guru_r2r; engine.motion_temporal_plans
 * makes the pair with motion's scales).  On such a pair ONE kernel (temporal_rt.hip) loads a tile of pixel columns, transforms over D,
 * filters at (z, 0, 0) for z < min(D, D'), transforms back over D' and stores, touching memory at the two ends only.  It takes
 *   every _u8 and _u8_dither call   d_work is not touched and may be NULL; a 1 x 1 block has no neighbour to diffuse into (the
 *                                   conditions of motion.c:781-785 are all false), so the dithered call's bytes are those of the _u8 call
 *                                   with out_mul = scalefactor normalization^2; dspfft_plan_set_u8_trc is honoured at both 8-bit ends
 *   every call with D' != D         d_in in `fwd`'s input layout, d_out in `inv`'s output layout; input and output must not overlap
 *   every float call whose filter needs positions (any filter but a pure quantiser): the stand-alone filter would derive them from a
 *                                   block-major offset; here positions are the block's own and minbuf_hw / block_depth are not consulted
 * For D' == D the 8-bit call may run in place (a tile reads all its frames before it writes any).  A float call on equal extents with no
 * filter or a pure quantiser runs the plans' own passes, as it always did.  -2, with the reason and nothing launched: a coefficient limit
 * below max(D, D') in any _topn / _limit entry, a length with a prime factor above 13, max(D, D') above 1024 (the narrowest tile of 16
 * columns in 64 KB of LDS), P no multiple of 4, float buffers off 16 bytes or 8-bit buffers off 4, more than 2^31 - 1 workgroups; -3 from a
 * library built without the HIP kernel. */

/* The same with motion's 8-bit samples at both ends (motion/motion.c:617-640 load, :760-776 store): d_in and d_out
 * hold uint8 samples in the plans' input / output element layout, d_work is a float buffer in the plans' working
 * layout.  When the first forward pass and the last inverse pass are planar specialised row passes they read the
 * bytes and write quantise(value * out_mul) themselves (5 B/sample each instead of 13); otherwise the conversions
 * run as separate sweeps (dspfft_u8_to_f32 / dspfft_f32_to_u8), which requires input, work and output layouts to be
 * identical and dense.
 * A clip of frames (2-D plans with one batch level, a column length that has a narrow-tile kernel, 8-bit row kernels at both ends) runs
 * in slices of frames whose float intermediate the last-level cache holds.  The first call that qualifies builds plans for a slice,
 * which the forward plan owns until it is destroyed: device allocations of their own, and -- unless DSPFFT_RT_STREAMS=1 -- one stream
 * and two events of the library's, on which every other slice runs; the call forks from hip_stream and joins it again before it
 * returns, also when it fails.  Calls on the same plan pair serialise on a mutex while they enqueue (they may use different buffers
 * and streams).  dspfft_plan_describe of the forward plan lists the slices from then on, in one more line.  The two switches,
 * DSPFFT_RT_SLICE (frames per slice; 0: never in slices) and DSPFFT_RT_STREAMS, are process-wide: read once, at the first such call. */
int dspfft_execute_roundtrip_u8(dspfft_plan fwd, dspfft_plan inv, const uint8_t *d_in, uint8_t *d_out, float *d_work, double out_mul,
                                const dspfft_motion_filter_params *filter, unsigned long long *d_coeffs_coded, void *hip_stream);
/* dspfft_execute_roundtrip_u8 with motion's -d: the final 8-bit store replaced by the dithered one (dspfft_motion_dither_u8 below, over the
 * inverse plan's extents -- `scaled` -- plane by plane: the last two transformed axes are the plane, the first of three and the batch axes
 * index planes; the contiguous axis must be the last).  Every path of the undithered call is taken alike (fused 8-bit load, fused column
 * roundtrip, a clip in slices, one 3-D block, scaled != block, the fused small-block kernel); the last inverse pass writes float into d_work
 * and the dither kernel writes the bytes.  d_work then holds the inverse transform's output (what was dithered), untouched by the dither.
 * d_coeffs_coded is counted as by the undithered call.  Same precision contract as dspfft_motion_dither_u8.  Single precision plans only. */
int dspfft_execute_roundtrip_u8_dither(dspfft_plan fwd, dspfft_plan inv, const uint8_t *d_in, uint8_t *d_out, float *d_work,
                                       double scalefactor, double normalization, const dspfft_motion_filter_params *filter,
                                       unsigned long long *d_coeffs_coded, void *hip_stream);
/* motion --linear on 8-bit video (motion/motion.c:632-633,768-769): a plan used as `fwd` of any dspfft_execute_roundtrip_u8* call decodes
 * every byte to linear light at its 8-bit load, a plan used as `inv` encodes at its 8-bit store (the dithered store included: the byte is the
 * encoded one, the diffused error stays the reference's c - byte / (normalization^2 scalefactor), :780).  trc: an
 * AVColorTransferCharacteristic id (dspfft_trc_from_name); 0, the default, resets: every call is then what it was, the same kernels and bytes.
 * On 8-bit samples the arithmetic is two tables (3 KB, built on the host with its libm when the function is set, on the device with the
 * plan until it is destroyed): the decode of a byte is one of 256 floats -- what the reference's default build (COEFF_PRECISION=F,
 * INTERMEDIATE_PRECISION=L) stores for it, bit for bit --, and encode + clamp + lround is a step function of the linear value, 255
 * thresholds found by bisection over the reference's lines in double; the byte is decided by comparisons with them alone.  No pow runs
 * on the device.  Every path of the 8-bit roundtrip takes the setting: the planar row ends and a clip in slices (kernels with the table
 * in LDS behind the line), one 3-D block, the fused small-block kernel with and without a coefficient limit, scaled != block (one block, and
 * a grid of blocks in its one kernel), the unfused
 * sweeps (dspfft_u8_to_f32_trc / dspfft_f32_to_u8_trc below; also for row kernels compiled at plan time) and the dithered store.  The result
 * equals dspfft_u8_to_f32_trc -> dspfft_execute_roundtrip -> dspfft_f32_to_u8_trc byte for byte.  A roundtrip on float buffers ignores it.
 * A narrowing to know of: a row kernel compiled at plan time (DSPFFT_JIT=1, a row length without a listed kernel) has no twin with tables, so
 * with a function set that end is converted by a sweep, and the call then has to meet the sweep's layout conditions (a dense work layout
 * for the output, identical input and work layouts for the input): a call that runs with trc 0 through such a kernel's fused end on another
 * layout is refused with -2 once a function is set, and a clip whose rows are such kernels is not walked in slices.
 * -1: an f64 plan, or a trc that is not built; -3: a library without the HIP kernels (and trc != 0). */
int dspfft_plan_set_u8_trc(dspfft_plan plan, int trc);

/* The two calls above with motion's --coeff-limit (motion/motion.c:652-668) between the forward transform and the filter: of every block's
 * coefficients -- as the forward plan writes them, which with motion's per-axis index-0 factors (dspfft_plan_set_axis_scale0, :644-647) are
 * the uniform-range coefficients the reference selects among -- the `keep` of largest magnitude stay and the rest become zero, before the
 * filter acts (:652 is ahead of :683).  The rule is dspfft_motion_topn_blocks' (below): the key is the bit pattern of |c|, ties at the
 * threshold go to the earliest in the block's own buffer order (z, then y, then x), NaNs are outside the contract.  The reference selects
 * over `mincomponent`, the largest component's buffer; for a smaller component the remainder is zeros, so per block this is a selection
 * over the block's own embedding.  preserve_dc = dc restores the block's DC as it was BEFORE the selection (:650, :734).
 * keep == 0 (the reference's `if(coeff_limit)`) or keep >= the block's embedding count: the call IS the plain one -- same kernels, same
 * bytes, every path of it, and d_topn_work may be NULL.  Otherwise:
 *   small blocks on the fused block pass (a volume's blocks, block-major stacks): ONE kernel as before, with the selection in the LDS tile
 *     between the forward and the inverse axes; needs no work buffer (dspfft_roundtrip_topn_work_bytes is 0 for such a plan pair)
 *   block-major stacks with DSPFFT_NO_BLOCK=1, clips of per-frame blocks, one 3-D block, scaled != block (count = the whole embedding,
 *     :657): the forward passes, dspfft_motion_topn_blocks over the blocks as contiguous runs of the working buffer, the stand-alone
 *     filter, the inverse passes.  For this call there is then NO fused column roundtrip and the clip does NOT run in slices: the
 *     selection needs every coefficient of a block before the filter sees one.  d_topn_work holds dspfft_roundtrip_topn_work_bytes.
 * Blocks that are no contiguous runs (interleaved batches; a volume's blocks on misaligned buffers) are refused (-2), and a library built
 * without the HIP selection kernels returns -3 for a keep in range, in both cases with nothing launched.  The dithered variant is dspfft_execute_roundtrip_u8_dither_limit (below). */
size_t dspfft_roundtrip_topn_work_bytes(dspfft_plan fwd, dspfft_plan inv);
int dspfft_execute_roundtrip_topn(dspfft_plan fwd, dspfft_plan inv, const float *d_in, float *d_out, const dspfft_motion_filter_params *filter,
                                  size_t keep, void *d_topn_work, size_t work_bytes, unsigned long long *d_coeffs_coded, void *hip_stream);
int dspfft_execute_roundtrip_u8_topn(dspfft_plan fwd, dspfft_plan inv, const uint8_t *d_in, uint8_t *d_out, float *d_work, double out_mul,
                                     const dspfft_motion_filter_params *filter, size_t keep, void *d_topn_work, size_t work_bytes,
                                     unsigned long long *d_coeffs_coded, void *hip_stream);

/* The coefficient limit as one argument, for the calls the two entries above do not cover: a rescaled block grid, and the dithered store.
 *   keep, d_work, work_bytes   the _topn entries' keep, d_topn_work and work_bytes (a grid needs no work buffer)
 *   outside_mul                read on a rescaled block grid only.  There the reference multiplies just the A = min(block, scaled) corner of
 *                              the M = max(block, scaled) embedding by the uniform-range factors (motion.c:644-647) and then ranks EVERY element
 *                              of the embedding (:652-668).  So, in the order e = (z MY + y) MX + x, an element ranks with: 0 outside `block`;
 *                              inside A the coefficient as `fwd` writes it (global scale and index-0 factors included); inside `block` but outside A
 *                              the coefficient WITHOUT `fwd`'s global scale and index-0 factors, times outside_mul.  1 for plans over the
 *                              reference's own three axes; 2 for the 2-D plans of a depth-1 grid, whose scale has absorbed the reference's unit
 *                              z axis (REDFT10 over one sample doubles).  A kept coefficient outside A only takes a slot: nothing reads it.
 * Key, ties, preserve_dc = dc and NaNs are the _topn entries' rules.  On the pairs those entries take, dspfft_execute_roundtrip_limit and
 * _u8_limit run the same path and give the same bytes.  On a grid pair all three run block_rescale_topn.hip's kernel -- the grid kernel with
 * unpruned forward passes and the selection in its LDS tile -- and keep >= MX MY MZ is the plain grid call.  _u8_dither_limit takes every pair
 * dspfft_execute_roundtrip_u8_dither takes (a clip is then not walked in slices) and equals the float-output limit call into d_work followed by
 * dspfft_motion_dither_u8 over it, byte for byte.
 * -1, nothing launched: cl NULL, keep == 0 (use the entries without a limit), outside_mul not finite or not > 0, and what the entries
 * above refuse; -2 / -3 as above. */
typedef struct { size_t keep; double outside_mul; void *d_work; size_t work_bytes; } dspfft_coeff_limit;
int dspfft_execute_roundtrip_limit(dspfft_plan fwd, dspfft_plan inv, const float *d_in, float *d_out, const dspfft_motion_filter_params *filter,
                                   const dspfft_coeff_limit *cl, unsigned long long *d_coeffs_coded, void *hip_stream);
int dspfft_execute_roundtrip_u8_limit(dspfft_plan fwd, dspfft_plan inv, const uint8_t *d_in, uint8_t *d_out, float *d_work, double out_mul,
                                      const dspfft_motion_filter_params *filter, const dspfft_coeff_limit *cl, unsigned long long *d_coeffs_coded,
                                      void *hip_stream);
int dspfft_execute_roundtrip_u8_dither_limit(dspfft_plan fwd, dspfft_plan inv, const uint8_t *d_in, uint8_t *d_out, float *d_work,
                                             double scalefactor, double normalization, const dspfft_motion_filter_params *filter,
                                             const dspfft_coeff_limit *cl, unsigned long long *d_coeffs_coded, void *hip_stream);

/* The fused small-block roundtrip on PACKED 8-bit pixels (motion -b 8x8x8 -q 20 -c pixel_format=rgb24, motion/motion.c:155-156: rgb24, bgr24,
 * rgba, bgra, argb, abgr, ya8): d_in and d_out hold `components` bytes per pixel, every byte a component, and each component of each pixel
 * block is a block of its own, as in the reference (:613-615) -- for the transform, for --coeff-limit (a selection per component block,
 * :652-668), for preserve_dc and for d_coeffs_coded, which counts the sum over the components.  ONE kernel (block_packed.hip): a thread reads
 * the NX * components contiguous bytes of a pixel block's line as whole dwords and picks the components apart in registers, so the clip moves
 * 2 * components bytes per pixel, where splitting it into planes, one planar call per plane and interleaving again moves about three times that.
 *   fwd, inv     the PLANAR small-block pair of dspfft_execute_roundtrip_u8's fused block pass (volume layout or block-major), planned over
 *                the clip in PIXELS; the call multiplies every stride and offset by `components`.  The same pair runs the planar call on a
 *                de-interleaved plane, and the bytes of this call EQUAL those of the planar call on each component's plane with that
 *                component's damp, boost and grey_add.
 *   filter       NULL: none, and only packed->components is read.  Otherwise packed->damp, boost and grey_add, indexed by BYTE POSITION inside
 *                the pixel, replace filter->damp, filter->boost and filter->grey_add (motion -D / -B r:g:b:a, :235-236,736), which are not
 *                read; every other field applies to all components (packed formats have no subsampling).
 *   cl           NULL: no --coeff-limit.  keep == 0 is refused (-1); keep >= the block's count is the plain call, same bytes; outside_mul,
 *                d_work and work_bytes are not read.
 *   dspfft_plan_set_u8_trc on either plan is honoured at that end, as in the planar call.
 * The call may run in place (d_in == d_out: a workgroup reads all its blocks before it writes any), is stream-ordered, allocates nothing and
 * uses no work buffer.  Nothing is launched when it fails:
 *   -1  a NULL plan, buffer or `packed`; an f64 plan; cl with keep == 0; bad filter parameters
 *   -2  components outside 2..4; a pair the fused block pass does not take (per-frame plans, one 3-D block); different extents in fwd and
 *       inv (a rescaled grid, motion -s: that pair is dspfft_execute_roundtrip_u8_packed_rescale's, below; -d is
 *       dspfft_execute_roundtrip_u8_packed_dither's and --spectrogram / --ispectrogram are dspfft_execute_spectrogram_u8_packed's /
 *       _ispectrogram_u8_packed's, all below); buffers off 4 bytes; a block whose `components` tiles plus the tables do not fit one workgroup's 64 KB of LDS -- of the listed extents that is
 *       16 x 16 x 16 at four components --; more than 2^31 - 1 workgroups
 *   -3  a library built without the HIP kernel */
typedef struct {
	int   components;                       /* 2, 3 or 4 bytes per pixel, every byte a component */
	float damp[4], boost[4], grey_add[4];   /* indexed by BYTE POSITION inside the pixel */
} dspfft_motion_packed;
int dspfft_execute_roundtrip_u8_packed(dspfft_plan fwd, dspfft_plan inv, const uint8_t *d_in, uint8_t *d_out, double out_mul,
                                       const dspfft_motion_filter_params *filter, const dspfft_motion_packed *packed,
                                       const dspfft_coeff_limit *cl /* NULL: no --coeff-limit */,
                                       unsigned long long *d_coeffs_coded, void *hip_stream);

/* The same with `scaled != block` over a grid of blocks (motion -b 8x8x8 -s 4x4x4 -c pixel_format=rgb24: motion/motion.c:488-499,535-552
 * with the components of :155-156,613-615): every component of every pixel block is transformed over `block` (REDFT10), filtered over
 * A = min(block, scaled) and transformed back over `scaled` (REDFT01) inside the embedding M = max(block, scaled) (:617), and the output
 * clip has other extents than the input clip.  ONE kernel (block_rescale_packed.hip: the rescaled grid's pruned phases between the packed
 * ends), so the call moves components * (input pixels + output pixels) bytes, where splitting the clip into planes, one planar grid call per
 * plane and interleaving again moves about three times that.  An entry of its own because the call is out of place by nature.
 *   fwd, inv     the PLANAR grid pair of dspfft_execute_roundtrip_u8 on a rescaled block grid (above: `fwd` cuts the input clip into blocks
 *                of `block`, `inv` the output clip into as many blocks of `scaled`; volume layout or block-major stacks; every extent 4, 8 or
 *                16, 2-D blocks up to 32), planned over the clips in PIXELS; the call multiplies every stride and offset by `components`.  The
 *                bytes of this call EQUAL those of the planar grid call on each component's plane with that component's damp, boost and
 *                grey_add, and d_coeffs_coded the sum of the planar counts.
 *   filter       the planar grid's: active = min(block, scaled), minbuf_hw and block_depth describe the embedding.  packed->damp, boost and
 *                grey_add, by BYTE POSITION, replace the filter's fields of those names, which are not read.  NULL: none, and only
 *                packed->components is read.
 *   dspfft_plan_set_u8_trc on either plan is honoured at that end, as in the planar call.
 * Stream-ordered, allocates nothing, uses no work buffer.  Nothing is launched when it fails, the reason in dspfft_last_error:
 *   -1  a NULL plan, buffer or `packed`; an f64 plan; bad filter parameters
 *   -2  components outside 2..4; a pair with equal extents (dspfft_execute_roundtrip_u8_packed, or _packed_frames); one block (howmany = 1)
 *       or a per-frame pair (full frames are dspfft_execute_roundtrip_u8_packed_frames's, with equal extents only); what the planar grid
 *       refuses of a pair: different ranks, an extent that is not 4, 8 or 16 (2-D: 32), kinds, axis orders, a stack against a volume,
 *       different numbers of blocks; buffers off 4 bytes; an input clip and an output clip whose byte ranges intersect (d_in == d_out is the
 *       simplest case); a pair whose `components` tiles (the embedding's planes and rows by min(block, scaled) columns) plus the tables do not
 *       fit one workgroup's 64 KB of LDS -- a 16 x 16 x 16 embedding with 16 columns on both sides at four components --; more than
 *       2^31 - 1 workgroups
 *   -3  a library built without the HIP kernel
 *   -4  a launch failure
 * --coeff-limit and -d are the two entries below (this one takes no limit).  Not implemented on a packed rescaled grid, each refused where a
 * call could ask for it: --spectrogram / --ispectrogram, -s over full frames or one block, float and padded (rgb0) formats. */
int dspfft_execute_roundtrip_u8_packed_rescale(dspfft_plan fwd, dspfft_plan inv, const uint8_t *d_in, uint8_t *d_out, double out_mul,
                                               const dspfft_motion_filter_params *filter, const dspfft_motion_packed *packed,
                                               unsigned long long *d_coeffs_coded, void *hip_stream);

/* dspfft_execute_roundtrip_u8_packed_rescale with motion --coeff-limit (motion -b 8x8x8 -s 4x4x4 --coeff-limit 16 -c pixel_format=rgb24): the same
 * pair, buffers, `packed` and filter, out of place (overlapping clips are refused), stream-ordered, no allocation, NO work buffer: cl->d_work and
 * cl->work_bytes are not read.  Every component block keeps its cl->keep coefficients of largest magnitude ahead of the filter; the reference
 * ranks the whole embedding M = max(block, scaled) (motion.c:652-668), so cl->outside_mul follows dspfft_coeff_limit's rule exactly as in
 * dspfft_execute_roundtrip_u8_limit on a rescaled grid.  ONE kernel (block_rescale_packed_limit.hip) on a WIDER tile than the plain call's: MX
 * columns per component block instead of min(block, scaled), because the selection reads the whole embedding; the forward passes run unpruned
 * (block_rescale_topn.hip's phases between the packed ends), the selection is topn_core.h's per component block, and with preserve_dc = dc the
 * restored DC is the one from before the selection, per component.
 * The bytes EQUAL those of dspfft_execute_roundtrip_u8_limit on the same planar grid pair on each component's plane with that component's damp,
 * boost and grey_add, and d_coeffs_coded the sum of the planar counts.  keep >= MX MY MZ is the plain call, with the same bytes.
 * Nothing is launched when it fails: dspfft_execute_roundtrip_u8_packed_rescale's codes and reasons under this entry's name, and
 *   -1  cl NULL, keep == 0, outside_mul not finite or not > 0
 *   -2  a pair whose `components` tiles of the WHOLE embedding plus the tables do not fit 64 KB of LDS: a 16 x 16 x 16 embedding at four components
 *       (three fit, one pixel block per workgroup); an embedding without a selection (none among the extents the grid takes)
 *   -3  a library built without the HIP kernel */
int dspfft_execute_roundtrip_u8_packed_rescale_limit(dspfft_plan fwd, dspfft_plan inv, const uint8_t *d_in, uint8_t *d_out, double out_mul,
                                                     const dspfft_motion_filter_params *filter, const dspfft_motion_packed *packed,
                                                     const dspfft_coeff_limit *cl, unsigned long long *d_coeffs_coded, void *hip_stream);

/* dspfft_execute_roundtrip_u8_packed_rescale with motion's -d, with or without --coeff-limit (cl as in the _limit entry above; NULL: no limit):
 * the same pair, buffers, `packed` and filter, out of place, stream-ordered, no allocation, NO work buffer.  scalefactor and normalization replace
 * out_mul (= scalefactor normalization^2) as in dspfft_execute_roundtrip_u8_dither.  ONE kernel (block_rescale_packed_dither.hip): the inverse's x
 * pass writes its SX floats back to the tile -- a component block is SX columns wide, MX with a limit --, the oz planes of oy x SX floats of every
 * tile block are the planes of the Floyd-Steinberg store, oy lanes walk one plane -- row y two pixels behind row y - 1, the errors handed down by
 * shuffles, each pixel with dither_core.h's arithmetic in the reference's order --, and the bytes leave through the packed store.  The error table
 * (2 KB) lies behind the tile, the transfer tables and the counter.
 * dspfft_plan_set_u8_trc on either plan is honoured as in dspfft_execute_roundtrip_u8_packed_dither.
 * The bytes EQUAL those of dspfft_execute_roundtrip_u8_dither (with cl: dspfft_execute_roundtrip_u8_dither_limit) on the same planar grid pair on
 * each component's plane with that component's damp, boost and grey_add, and d_coeffs_coded the sum of the planar counts.
 * Nothing is launched when it fails: the codes and reasons of the two entries above under this entry's name, and
 *   -1  scalefactor or normalization not finite or not > 0; cl non-NULL with keep == 0 or a bad outside_mul
 *   -2  a pair whose tile, tables and error table do not fit 64 KB of LDS even with one pixel block per workgroup
 *   -3  a library built without the HIP kernel */
int dspfft_execute_roundtrip_u8_packed_rescale_dither(dspfft_plan fwd, dspfft_plan inv, const uint8_t *d_in, uint8_t *d_out, double scalefactor, double normalization,
                                                      const dspfft_motion_filter_params *filter, const dspfft_motion_packed *packed,
                                                      const dspfft_coeff_limit *cl /* NULL: no --coeff-limit */,
                                                      unsigned long long *d_coeffs_coded, void *hip_stream);

/* The small-block call on FULL FRAMES of packed pixels -- the reference's default block -b 0x0x1, what `motion -q 20 in.png out.png` or
 * `motion -c pixel_format=rgb24` on a clip runs: every component of every frame is one block (:613-615).  An entry of its own because the
 * passes of full frames need a float work buffer, which the small-block entry has no argument for.
 *   fwd, inv     the caller's in-place, dense, interleaved f32 pair of rank 2 over [F][H][W][C], the plans of the full-frame spectrogram calls
 *                below: axes {H: stride W C, W: stride C}, batch levels {C: stride 1} and, for F > 1, {F: stride H W C}
 *                (dspfft_plan_guru_r2r: REDFT10; the inverse REDFT01 with dspfft_plan_guru_r2r_ordered(..., 1), so that its column pass
 *                begins it), with motion's scales.
 *   d_work       F H W C floats, sharing the layout element for element.  d_in == d_out is allowed.
 *   filter       NULL: none, and only packed->components is read.  Otherwise active = (1, H, W), minbuf_hw = (H, W) and block_depth = 1 are the
 *                call's own (those fields are checked, then not read); the band, the thresholds, preserve_dc and the quantiser are the
 *                caller's, and packed->damp, boost and grey_add, by byte position, replace the filter's fields of those names exactly as above.
 * The sequence is dspfft_execute_roundtrip_u8's on that pair: the forward row pass into d_work -- with the interleaved 8-bit row load where
 * the pass has one and every line of bytes starts at a multiple of 4, after dspfft_u8_to_f32 otherwise --; the forward column pass, the filter
 * and the inverse column pass as ONE kernel where both passes have the same listed column kernel, that kernel has the twin with the filter of
 * packed pixels (spec_inst_rt_packed_a/b.hip; kernels compiled at plan time have none) and d_work is 16-byte aligned, else as forward column
 * pass, dspfft_motion_filter_packed (below), inverse column pass; the inverse row pass with the interleaved 8-bit store where it has one, else
 * dspfft_f32_to_u8(out_mul).  No filter, or one in which nothing but the quantiser acts on any component, runs in the planar fused kernel: the
 * bytes are the same.  DSPFFT_NO_FUSED_ROUNDTRIP=1 selects the unfused column sequence.  The bytes and the coded count EQUAL those of the
 * composition dspfft_u8_to_f32 -> dspfft_execute(fwd) -> dspfft_motion_filter_packed -> dspfft_execute(inv) -> dspfft_f32_to_u8(out_mul).
 * dspfft_plan_set_u8_trc on either plan (motion --linear) is honoured by the flat sweep dspfft_u8_to_f32_trc / dspfft_f32_to_u8_trc at that
 * end, which then does not ride on the row pass.  A filtered call whose work buffer holds 2^31 elements or more runs the UNFUSED column
 * sequence: the fused kernel addresses the clip with 31-bit offsets, the stand-alone kernel's are frame-local.
 * Stream-ordered, allocates nothing.  Nothing is launched when it fails, the reason in dspfft_last_error:
 *   -1  a NULL plan, buffer, d_work or `packed`; an f64 plan; bad filter parameters
 *   -2  components outside 2..4, or not the count of the plans' unit-stride batch level; a small-block pair (that is
 *       dspfft_execute_roundtrip_u8_packed); rank 3 (one 3-D block, -b 0x0x0); different extents in fwd and inv (-s); a pair that is not the
 *       dense in-place layout above with REDFT10 in fwd, REDFT01 in inv and inv running its column pass first; a frame of 2^32 samples or more
 *   -3  a library built without the HIP kernels
 * -d is dspfft_execute_roundtrip_u8_packed_frames_dither's (below).  Not implemented on packed full frames, each refused where a call could
 * ask for it: --coeff-limit (a component's frame is no contiguous run: this entry takes no limit), -s, one 3-D block, float and padded (rgb0) formats. */
int dspfft_execute_roundtrip_u8_packed_frames(dspfft_plan fwd, dspfft_plan inv, const uint8_t *d_in, uint8_t *d_out, float *d_work, double out_mul,
                                              const dspfft_motion_filter_params *filter, const dspfft_motion_packed *packed,
                                              unsigned long long *d_coeffs_coded, void *hip_stream);

/* dspfft_execute_roundtrip_u8_packed with motion's -d (motion -b 8x8x8 -q 20 -d on rgb24: motion.c:778-787 inside the loop over components,
 * :613-615): that entry's contract in every respect but the store -- the same planar small-block pair, 2, 3 or 4 components, per-byte damp / boost
 * / grey_add, cl, dspfft_plan_set_u8_trc at either end (the dithered byte is then the encoded one, as in dspfft_motion_dither_u8_trc), in place
 * allowed, stream-ordered, no allocation and NO work buffer.  scalefactor and normalization replace out_mul (= scalefactor normalization^2), as in
 * dspfft_execute_roundtrip_u8_dither: the error of a pixel is c - byte / (normalization^2 scalefactor).
 * ONE kernel (block_packed_dither.hip), no float intermediate: when the inverse's y pass ends, the z planes of a tile's component blocks are the
 * planes of the Floyd-Steinberg store and lie in LDS whole.  The inverse's x pass writes its floats back to the tile (bit for bit what the planar
 * dithered call leaves in d_work), one thread per plane walks it in raster order (dither_core.h: the arithmetic and its precision contract are
 * dspfft_motion_dither_u8's) leaving each byte where its float was, and the bytes leave through the packed store: 2 * components bytes per pixel.
 * The bytes EQUAL those of dspfft_execute_roundtrip_u8_dither (with cl: _dither_limit) on the same pair on each component's plane with that
 * component's damp, boost and grey_add, and d_coeffs_coded the sum of the planar counts.
 * A plane is a dependent chain of NY NX steps in double on one lane, so blocks with few, large planes (1 x 32 x 32) leave most of a workgroup
 * idle during the dither; measured only on 8 x 8 x 8 and 1 x 8 x 8 blocks (profiles/r22_motion_packed_dither.txt).
 * Nothing is launched when it fails: dspfft_execute_roundtrip_u8_packed's codes and reasons under this entry's name, and
 *   -1  scalefactor or normalization not finite or not > 0
 *   -2  a tile whose component blocks, tables, error table (2 KB) and error rows (NX doubles per dither lane) do not fit 64 KB of LDS;
 *       different extents in fwd and inv: -d on a packed rescaled grid is not implemented by this entry (its tile has one block's extents); that
 *       call is dspfft_execute_roundtrip_u8_packed_rescale_dither's
 *   -3  a library built without the HIP kernel
 * Not implemented with -d on packed pixels: one 3-D block, float and padded (rgb0) formats. */
int dspfft_execute_roundtrip_u8_packed_dither(dspfft_plan fwd, dspfft_plan inv, const uint8_t *d_in, uint8_t *d_out, double scalefactor, double normalization,
                                              const dspfft_motion_filter_params *filter, const dspfft_motion_packed *packed,
                                              const dspfft_coeff_limit *cl /* NULL: no --coeff-limit */,
                                              unsigned long long *d_coeffs_coded, void *hip_stream);

/* dspfft_execute_roundtrip_u8_packed_frames with motion's -d: the same pair, buffers, filter and sequence up to the last inverse pass -- the
 * fused packed column roundtrip, the unfused sequence (DSPFFT_NO_FUSED_ROUNDTRIP=1) and the quantiser-only shortcut are taken as there --, but the
 * inverse row pass writes FLOAT into d_work (no 8-bit row end, no dspfft_f32_to_u8) and dspfft_motion_dither_u8_packed (below) over
 * [F][H][W][C] -- n = {1, H, W}, nblocks = {F, 1, 1}, block_step = {H W} -- writes the bytes.  d_work afterwards holds what was dithered.
 * A transfer characteristic on `inv` is applied by the dither's trc variant, one on `fwd` by the flat sweep as in the undithered call.
 * d_in == d_out is allowed.  The floats in d_work and the coded count EQUAL those of the composition dspfft_u8_to_f32 -> dspfft_execute(fwd) ->
 * dspfft_motion_filter_packed -> dspfft_execute(inv), and the bytes those of dspfft_motion_dither_u8_packed over them.
 * Nothing is launched when it fails: the undithered entry's codes and reasons under this entry's name, and
 *   -1  scalefactor or normalization not finite or not > 0
 *   -2  what dspfft_motion_dither_u8_packed refuses of the frames, with its reason: a width above the wavefront kernel's LDS rings (about 9000) */
int dspfft_execute_roundtrip_u8_packed_frames_dither(dspfft_plan fwd, dspfft_plan inv, const uint8_t *d_in, uint8_t *d_out, float *d_work, double scalefactor,
                                                     double normalization, const dspfft_motion_filter_params *filter, const dspfft_motion_packed *packed,
                                                     unsigned long long *d_coeffs_coded, void *hip_stream);

/* motion --spectrogram and --ispectrogram (motion/motion.c:617-776 with `spec` / `ispec` set) as one call per clip: the two halves of
 * the roundtrip above, each with ONE plan.
 *   spectrogram   load (:621-625) -> REDFT10 over `fwd`'s extents (`fwd` carries motion's index-0 factors, dspfft_plan_set_axis_scale0,
 *                 :647) -> dc = the block's element 0 (:650) -> filter (:683-744, d_coeffs_coded as above) -> encode (:755-771) -> store:
 *                 8-bit clamp + lround (:776), float pel / 255 (:774).  mode: abs, shift, flat or copy.
 *   ispectrogram  load (the 8-bit sample, or the float sample * 255 as a float product, :623) -> decode (:627-630) -> filter -> REDFT01
 *                 over `inv`'s extents (`inv` carries :751's factors and the global scale) -> store as dspfft_execute_roundtrip_u8 stores:
 *                 quantise(value * out_mul), out_mul = scalefactor normalization^2; the float form stores value * out_mul / 255.
 *                 mode: shift, flat or copy (the reference has no abs type here: -2).
 * The _f32 forms are motion's float_pixels (planar float formats, what the reference picks for flat and copy by default), not raw
 * coefficients.  sp->c is :568's constant (spectrogram, shift) or :569's (ispectrogram, shift) and ignored otherwise: for abs every block's
 * own c = 255 / log1p(|dc scalefactor normalization|) (:755) is derived on the device from that block's DC, with no host round trip.  A
 * block whose DC is exactly 0 under abs is outside the contract (the reference computes 255 / 0 there): the call succeeds and that block's
 * samples are unspecified.  The 8-bit abs / shift encode runs in single precision wherever that decides the byte and in double next to a
 * rounding boundary (motion_filter.h): the byte is the double evaluation's for every coefficient.  The filter is the roundtrip's, `active` = the block; filter == NULL: none.
 * Small-block plans (every extent 4, 8 or 16, 2-D blocks up to 32, x contiguous; the blocks of a volume via dspfft_plan_guru_r2r or a
 * block-major stack via dspfft_plan_many_r2r -- the plans the fused block roundtrip takes): each call is ONE kernel, 2 B/sample on 8-bit
 * pixels.  d_in is read in the plan's input layout and d_out written in its output layout, so in the volume layout every block's
 * spectrogram lands where the block was (:795-802).  d_work is not touched and may be NULL; float buffers must be 16-byte aligned and 8-bit
 * ones 4-byte (-2 otherwise); d_in == d_out is allowed (a workgroup has read its blocks before it writes them).
 * Every other plan (motion's default -b 0x0x1 over a clip: a 2-D plan with a batch of frames; one 3-D block): the plan must be in place on
 * one layout (input strides = output strides, x contiguous, planes of a block one pitch apart, at most one batch level, -2 otherwise),
 * which d_in, d_work and d_out share element for element.  spectrogram: the forward passes -- the first with the plan's fused 8-bit row
 * load where it has one, after dspfft_u8_to_f32 otherwise -- into d_work, then dspfft_motion_spec_blocks_* (below) once over all blocks
 * of the batch; ispectrogram: dspfft_motion_ispec_blocks_* once into d_work, then the inverse passes, the last with the plan's fused
 * 8-bit store where it has one (dspfft_f32_to_u8 otherwise, which needs a dense layout).  A float-pixel call converts its linear end with
 * one more sweep of the same kernels.  d_work is required (-1).
 * Refused with -2, the reason in dspfft_last_error and nothing launched -- each a stated follow-up: a plan with dspfft_plan_set_u8_trc set
 * (--linear with a spectrogram), an f64 plan, abs passed to an ispectrogram call, misaligned buffers with a small-block plan.  A plan pair is
 * not involved, so motion's `scaled != block` (-s with --spectrogram) does not arise: a caller who wants it runs the forward plan and encodes
 * the scaled corner with dspfft_motion_spec_blocks_*.  There is no coefficient-limit and no dithered variant (the reference disables -d with
 * --spectrogram).  -3 from a library built without the HIP kernels. */
typedef struct { int mode; double scalefactor, normalization, c; } dspfft_motion_spec_params;   /* mode: DSPFFT_MOTION_* (below) */
int dspfft_execute_spectrogram_u8(dspfft_plan fwd, const uint8_t *d_in, uint8_t *d_out, float *d_work, const dspfft_motion_spec_params *sp,
                                  const dspfft_motion_filter_params *filter, unsigned long long *d_coeffs_coded, void *hip_stream);
int dspfft_execute_spectrogram_f32(dspfft_plan fwd, const float *d_in, float *d_out, float *d_work, const dspfft_motion_spec_params *sp,
                                   const dspfft_motion_filter_params *filter, unsigned long long *d_coeffs_coded, void *hip_stream);
int dspfft_execute_ispectrogram_u8(dspfft_plan inv, const uint8_t *d_in, uint8_t *d_out, float *d_work, const dspfft_motion_spec_params *sp,
                                   const dspfft_motion_filter_params *filter, double out_mul, unsigned long long *d_coeffs_coded, void *hip_stream);
int dspfft_execute_ispectrogram_f32(dspfft_plan inv, const float *d_in, float *d_out, float *d_work, const dspfft_motion_spec_params *sp,
                                    const dspfft_motion_filter_params *filter, double out_mul, unsigned long long *d_coeffs_coded, void *hip_stream);

/* The two 8-bit calls above on PACKED pixels -- what the reference runs them on: with --spectrogram / --ispectrogram and no -c it takes an
 * 8-bit RGB format (motion.c:313-318), and every such format but gbrp is packed.  d_in and d_out hold packed->components (2, 3 or 4) bytes
 * per pixel, every byte a component, and each component of each block is a block of its own (:613-615): for the transform, for the block's
 * DC and abs's c = 255 / log1p(|dc scalefactor normalization|) (:650,755), for preserve_dc, and for d_coeffs_coded, which counts the sum
 * over the components.  packed->damp, boost and grey_add, indexed by byte position, replace the filter's fields of those names as in
 * dspfft_execute_roundtrip_u8_packed; filter == NULL: none, and only packed->components is read.  Modes as above (abs is refused on the
 * inverse side).  Two plan families, told apart by the plan:
 *   small blocks   the PLANAR small-block plan over the clip in PIXELS (the plans dspfft_execute_roundtrip_u8_packed takes: volume layout
 *                  or block-major stack, extents 4 / 8 / 16, 2-D blocks up to 32); the call multiplies every stride and offset by
 *                  `components`.  ONE kernel (block_spec_packed.hip): a thread reads or writes the NX * components bytes of a pixel
 *                  block's line as whole dwords and picks the components apart in registers.  The bytes EQUAL those of the planar call
 *                  with the same plan on each component's plane with that component's damp, boost and grey_add.  d_work is not touched
 *                  and may be NULL; the buffers must be 4-byte aligned.
 *   full frames    (motion's default -b 0x0x1) the caller's in-place, dense, interleaved f32 plan of rank 2 over [F][H][W][C]: axes
 *                  {H: stride W C, W: stride C}, batch levels {C: stride 1} and, for F > 1, {F: stride H W C} (dspfft_plan_guru_r2r;
 *                  the inverse with dspfft_plan_guru_r2r_ordered(..., 1), so that its row pass ends it).  d_work is required: F H W C
 *                  floats, sharing the layout element for element.  spectrogram: the plan's passes into d_work -- the first with the
 *                  interleaved 8-bit row load where the plan has one and every line of bytes starts at a multiple of 4, after
 *                  dspfft_u8_to_f32 otherwise --, then dspfft_motion_spec_blocks_u8_packed once over all frames; ispectrogram:
 *                  dspfft_motion_ispec_blocks_u8_packed into d_work, then the passes, the last with the 8-bit store where it has one,
 *                  else dspfft_f32_to_u8.  The bytes EQUAL those of that composition with dspfft_execute.
 * Both are stream-ordered, allocate nothing and allow d_in == d_out.  Nothing is launched when they fail:
 *   -1  a NULL plan, buffer, sp or packed; a bad mode; bad filter parameters; the wrong transform kind on an axis; a full-frame plan
 *       without d_work
 *   -2  components outside 2..4; an f64 plan; a plan with dspfft_plan_set_u8_trc set; abs on the inverse side; small blocks: buffers off
 *       4 bytes, a tile of `components` blocks that does not fit a workgroup's 64 KB of LDS (of the listed extents 16 x 16 x 16 at
 *       four components), more than 2^31 - 1 workgroups; full frames: a plan whose unit-stride batch level does not count
 *       packed->components, or that is not the dense in-place layout above; a plan of rank 3 that is no small-block plan (one 3-D
 *       block, -b 0x0x0: a stated follow-up)
 *   -3  a library built without the HIP kernels */
int dspfft_execute_spectrogram_u8_packed(dspfft_plan fwd, const uint8_t *d_in, uint8_t *d_out, float *d_work, const dspfft_motion_spec_params *sp,
                                         const dspfft_motion_filter_params *filter, const dspfft_motion_packed *packed,
                                         unsigned long long *d_coeffs_coded, void *hip_stream);
int dspfft_execute_ispectrogram_u8_packed(dspfft_plan inv, const uint8_t *d_in, uint8_t *d_out, float *d_work, const dspfft_motion_spec_params *sp,
                                          const dspfft_motion_filter_params *filter, const dspfft_motion_packed *packed, double out_mul,
                                          unsigned long long *d_coeffs_coded, void *hip_stream);

/* spec and ispec on 8-bit images (spec/spec.c:63-139 and spec/ispec.c:84-167 with an 8-bit reader and writer) as one call each way, device
 * memory to device memory:
 *   spec_u8   bytes -> REDFT10 over h x w with `channels` interleaved signals -> display encoding (dspfft_spec_encode's codes; the divisors
 *             come from the first pixel on the device) -> bytes clamp(lround(255 e)).  d_signmap (NULL ok; sign type abs only): the same
 *             sweep also writes the `sign` preset's bytes (spec.h:75: linear, saturate, range one, gain 1), the companion image ispec -m
 *             reads.  d_dc (device, NULL ok): the `channels` doubles of the header's "DC" property (spec.c:66-68).
 *   ispec_u8  bytes (b / 255 as the reader gives it) [+ sign map, ispec.c:91-95] -> unsign, unscale, / gain, optional DC restore (dc: host
 *             memory, as dspfft_ispec_decode's; needed for range dc / dcs and for restore_dc) -> REDFT01 -> bytes quantise(255 p).
 * The plans are the caller's and carry the normalisation: `fwd` a dense in-place f32 plan of rank 2 in the default pass order with scale
 * 1 / (255 * 2wh) and 1 / sqrt 2 at output index 0 of both axes (spec.c:70-78 on (float)byte); `inv` the REDFT01 plan made with
 * dspfft_plan_many_r2r_ordered(..., 1), so that the row pass ends it, with ispec.c:153-159's factors (sqrt 2 at input index 0 of both axes,
 * scale 1/2).  Both: howmany = channels (<= 4), stride = channels, dist = 1.
 * Sweeps: the row pass reads (writes) the bytes itself where it has an 8-bit end -- planar lines and the interleaved RGB lines of 3840,
 * 1920, 7680, 960, 512 and 256 pixels, with the image 4-byte aligned and w * channels a multiple of 4; dspfft_u8_to_f32 / dspfft_f32_to_u8
 * otherwise (runtime-geometry lines, other channel counts, plans with a window, modulation or alternating sign, frames that run on the
 * split passes) -- then the column pass in d_work and ONE sweep for the encoding and its store (or, first, the load and its decoding).
 * The bytes, the sign map and the DC values are those of dspfft_u8_to_f32 -> dspfft_execute -> dspfft_spec_encode -> dspfft_f32_to_u8(255)
 * (once more with the sign preset), and of the upload of b / 255 -> dspfft_ispec_signmap -> dspfft_ispec_decode -> dspfft_execute ->
 * dspfft_f32_to_u8(255).  d_in == d_out is allowed.  Stream-ordered, no allocation: both calls can sit in a captured graph.
 * Refused with -2, the reason in dspfft_last_error and nothing launched: an f64 plan, a plan of another rank, kind, layout or pass order,
 * more than 4 channels, a sign map with a sign type other than abs, range dc / dcs or restore_dc without dc, d_work == NULL.  -3 from a
 * library built without the HIP kernels. */
typedef struct { double gain; int rangetype, scaletype, signtype; } dspfft_spec_image_params;   /* codes as dspfft_spec_encode */
int dspfft_execute_spec_u8(dspfft_plan fwd, const uint8_t *d_in, uint8_t *d_out, uint8_t *d_signmap, float *d_work, double *d_dc,
                           const dspfft_spec_image_params *sp, void *hip_stream);
int dspfft_execute_ispec_u8(dspfft_plan inv, const uint8_t *d_in, const uint8_t *d_signmap, uint8_t *d_out, float *d_work, const double *dc,
                            int restore_dc, const dspfft_spec_image_params *sp, void *hip_stream);

/* Replaces fftw(destroy_plan). */
void dspfft_destroy_plan(dspfft_plan plan);

/* Human-readable list of the passes a plan runs (kernel shape, radices, tile, LDS bytes). */
int dspfft_plan_describe(dspfft_plan plan, char *buf, size_t buflen);

/* Algorithmic bytes one execute moves (read once + write once per transformed sample, 8 B/sample
 * for f32, 16 for f64) -- the numerator of bench.py's roofline figure. */
size_t dspfft_plan_algorithmic_bytes(dspfft_plan plan);

const char *dspfft_last_error(void);
const char *dspfft_version(void);

/* ---- device-side helpers around the transform ---- */

/* scan/scan_methods.c:77-115 (scan_zigzag): lin[i - first] = y*w + x of scan index i, i in [first, first+count).
 * d_lin: device uint32 array.  Integer, bit-exact. */
int dspfft_scan_zigzag(uint32_t *d_lin, uint32_t w, uint32_t h, uint64_t first, uint64_t count, void *hip_stream);

/* scan/scan.c:429-432,445: recon = 0 everywhere except the `count` listed pixels (all c channels copied
 * from coeffs), DC pixel cleared. */
int dspfft_scan_scatter(float *d_recon, const float *d_coeffs, const uint32_t *d_lin, uint64_t count,
                        uint64_t npixels, int channels, void *hip_stream);

/* The whole per-frame step of scan's hot loop (scan/scan.c:429-432,445-459) as one fused execution of an
 * inverse plan:   d_acc += plan( d_in restricted to elements e with d_ids[e / elems_per_id] == id )
 * The first pass masks while loading (no zeroed `reconstruction` buffer, no scatter), the last pass
 * adds into d_acc while storing (no `image` buffer, no separate sum pass): 21.3 B/sample of traffic for
 * a 3-channel image instead of 32.  d_work: scratch with the plan's output layout.  d_ids == NULL
 * disables masking.  elems_per_id = channels for the image tools' interleaved buffers.
 * Plans with split column passes (8K-class frames) skip the column tiles none of whose coefficients belongs to `id` and keep
 * per-tile flags for the row pass in scratch owned by the plan: run one fused step per plan at a time (concurrent streams take
 * one plan each); d_work then holds garbage in the skipped tiles, as scratch may. */
int dspfft_execute_masked_accumulate(dspfft_plan plan, const float *d_in, float *d_work, float *d_acc,
                                     const uint32_t *d_ids, uint32_t id, int elems_per_id, void *hip_stream);
/* The same step over a RANGE of owner ids:
 *     d_acc += plan( d_in restricted to elements e with lo <= d_ids[e / elems_per_id] < hi )
 * With an owner-index table (dspfft_scan_owner_index, or a magnitude / file index) one call adds every scan index of [lo, hi): scan's
 * --offset fill (scan/scan.c:389-417), an inverted-order frame (:424), or the prefix a frame-range shard starts from (dist.py
 * FrameShardedScan).  hi <= lo selects nothing.  The id 0xFFFFFFFF (the DC pixel, pixels no index owns) is never selected, whatever hi:
 * the reference clears DC before every inverse (scan.c:406,445), so the caller's table need not mark it.  d_ids must not be NULL.
 * A table prepared with dspfft_plan_scan_prepare is used as for one id; its 1- or 2-byte element ids saturate at 0xff / 0xffff, and both
 * ends of the range are clamped to that value, which drops nothing (such a table exists only while every other id lies below it).
 * The tile (min, max) skip of a prepared table applies to single ids only: a range reads the tiles' ids.
 * dspfft_execute_masked_accumulate(..., id, ...) is this call on [id, id + 1), bit for bit. */
int dspfft_execute_masked_accumulate_range(dspfft_plan plan, const float *d_in, float *d_work, float *d_acc,
                                           const uint32_t *d_ids, uint32_t lo, uint32_t hi, int elems_per_id, void *hip_stream);
int dspfft_execute_masked_accumulate_range_f64(dspfft_plan plan, const double *d_in, double *d_work, double *d_acc,
                                               const uint32_t *d_ids, uint32_t lo, uint32_t hi, int elems_per_id, void *hip_stream);

/* d_ids[y*w+x] = (zigzag scan index of (y,x)) / step -- the output frame (scan/scan.c:421-427) that
 * reconstructs coefficient (y,x); the DC pixel gets 0xFFFFFFFF (it is pre-added, scan.c:377-383,445). */
int dspfft_scan_zigzag_frame_ids(uint32_t *d_ids, uint32_t w, uint32_t h, uint64_t step, void *hip_stream);

/* ---- the other scan methods on the device (scan/scan_methods.c:59-67,122-208,240-331), SURVEY.md 8f #3 ----
 * Method numbers follow host/scan_orders.h.  Every generator is bit-exact against the reference's (integer arithmetic; radial's
 * rint(hypot) is evaluated exactly).  How a frame loop uses them:
 *   all methods but box: dspfft_scan_frame_ids once, then dspfft_execute_masked_accumulate(..., frame, ...) per output frame;
 *   box (a pixel can belong to several scan indices, and its first leg runs out of the image on tall frames): per frame
 *     dspfft_scan_coords of the frame's scan indices -> dspfft_scan_stamp(ids, ..., frame) -> the same fused execution;
 *   magnitude (needs the coefficients): dspfft_scan_magnitude_index -> dspfft_scan_index_to_frame_ids;
 *   file: parsed on the host (host/scan_orders.c scan_order_read_file), uploaded as an index array or as coordinate lists. */
enum {
	DSPFFT_SCAN_HORIZONTAL = 0, DSPFFT_SCAN_VERTICAL = 1, DSPFFT_SCAN_ZIGZAG = 2, DSPFFT_SCAN_ROW = 3, DSPFFT_SCAN_COLUMN = 4,
	DSPFFT_SCAN_DIAGONAL = 5, DSPFFT_SCAN_MIRROR = 6, DSPFFT_SCAN_BOX = 7, DSPFFT_SCAN_IBOX = 8, DSPFFT_SCAN_RADIAL = 9, DSPFFT_SCAN_IRADIAL = 10
};
/* number of scan indices (scan_context.c:30 via the method's limit function) and the most coordinates one index yields (host arithmetic) */
uint64_t dspfft_scan_limit(int method, uint32_t w, uint32_t h);
uint64_t dspfft_scan_max_interval(int method, uint32_t w, uint32_t h);
/* entries per scan index in the coordinate lists below: max_interval, + 1 for box / ibox (the entry scan.c:346 over-allocates; ibox's
 * index 0 emits w + h coordinates against max_interval = w + h - 1, scan_methods.c:135-144,502) */
uint64_t dspfft_scan_coord_slots(int method, uint32_t w, uint32_t h);
/* d_index[y*w+x] = the scan index that yields pixel (y,x); every method except box (no single owner) */
int dspfft_scan_owner_index(uint32_t *d_index, int method, uint32_t w, uint32_t h, void *hip_stream);
/* d_ids[y*w+x] = owner index / step, the DC pixel 0xFFFFFFFF: the generalisation of dspfft_scan_zigzag_frame_ids (which it calls for zigzag) */
int dspfft_scan_frame_ids(uint32_t *d_ids, int method, uint32_t w, uint32_t h, uint64_t step, void *hip_stream);
/* coordinate lists: for scan indices [first, first+count), slot j < dspfft_scan_coord_slots of index i holds y*w+x of its j-th coordinate,
 * or 0xFFFFFFFF (slot beyond the index's interval, or a box coordinate past the end of the image); all methods but radial / iradial.
 * d_lin holds count * dspfft_scan_coord_slots entries. */
int dspfft_scan_coords(uint32_t *d_lin, int method, uint32_t w, uint32_t h, uint64_t first, uint64_t count, void *hip_stream);
/* d_ids[d_lin[t]] = frame_id for every valid entry (the DC pixel is left alone): builds the mask of ONE frame from coordinate lists;
 * ids of earlier frames need no clearing as long as frame ids are not reused (initialise d_ids to 0xFFFFFFFF once) */
int dspfft_scan_stamp(uint32_t *d_ids, const uint32_t *d_lin, uint64_t nslots, uint32_t frame_id, void *hip_stream);
/* in place: ids[p] = index[p] / step, DC pixel 0xFFFFFFFF (for index arrays from dspfft_scan_magnitude_index or a `file` order) */
int dspfft_scan_index_to_frame_ids(uint32_t *d_ids, uint64_t npixels, uint64_t step, void *hip_stream);
/* scan_methods.c:240-296: d_index[p] = scan index of pixel p when pixels are ordered by descending magnitude key
 * (sum_z |c|, x sqrt2 per non-zero index, optionally quantised by qfactor; 0 = off), INCLUDING the reference's grouping rule (an
 * element whose key differs from its predecessor's still joins the predecessor's index; the next element opens a new one).
 * Ties: the reference leaves their order to qsort; here equal keys keep raster order (stable sort) -- documented, deterministic.
 * Synchronises the stream; *limit receives the number of scan indices.  d_work: dspfft_scan_magnitude_work_bytes(w, h) bytes. */
size_t dspfft_scan_magnitude_work_bytes(uint32_t w, uint32_t h);
int dspfft_scan_magnitude_index(uint32_t *d_index, const float *d_coeffs, uint32_t w, uint32_t h, int channels, double qfactor,
                                void *d_work, size_t work_bytes, uint32_t *limit, void *hip_stream);

/* ---- scan's output frames on the device (scan/scan.c:366-375,379-417,419-536), HIP-only entry points ----
 * The frame scan hands its encoder each output step: AV_PIX_FMT_GBRPF32LE, three planes of W' = w (1 + visualize) by H' = h (1 + intermediates)
 * floats in plane order G, B, R (channel z = 0, R, is plane 2; z = 1 plane 0; z = 2 plane 1), dspfft_scanframes_frame_floats floats in all.
 * Panels: top-left the reconstruction `sum`; top-right (-v) every visited coefficient, 1.0 or with -s its spectrogram value
 * sign(scale(c * spec_normalization_2d(x, y) * gain) / max) in double (speclib.c:133-174; gain and the DC pixel's largest channel rounded to
 * float first, as spec_create's `coeff` arguments round them); bottom-left (-i) this frame's inverse plus DC, ((image + dc) - min) / (max - min)
 * in float with min, max = 0, 1 or (-M) the frame's per-channel min / max plus DC (an all-zero image gives NaN under -M, as the reference
 * writes); bottom-right (-v -i) this frame's coefficients alone.  Panels the reference never clears keep their contents between frames.
 * Per run: begin (clears the frame, as ffapi_clear_frame, and sets the scaler from the DC pixel of d_coeffs), mark the fill's indices
 * (current = 0), then per frame: mark the frame's indices (current = 1), the fused step, compose.
 * With -i the fused step must add into an IMAGE buffer of w h 3 floats holding -0.0f (0x80000000) instead of d_sum: -0 + v == v, so the
 * buffer receives exactly what the fused store would have added to the sum; compose then adds it to d_sum (the same float as the fused
 * path) and refills it with -0.0f for the next frame.  The caller fills it with -0.0f once.  All buffers interleave channels (HWC).
 * Stream-ordered, no host synchronisation except dspfft_scanframes_parity.  Frame offsets are 64-bit. */
typedef struct {
	int visualize;                          /* -v: the right-hand panels */
	int spectrogram;                        /* -s (implies -v): spectrogram values instead of 1.0 */
	int intermediates;                      /* -i: the bottom panels */
	int max_intermediates;                  /* -M (implies -i): the bottom-left panel normalised by its own min / max */
	double spec_gain;                       /* --spec-gain; 0: 127.5 sqrt(4 w h) (scan.c:367-368) */
	int spec_scaletype;                     /* speclib's scaletype: 0 none (= log), 1 linear, 2 log */
	int spec_signtype;                      /* speclib's signtype: 0 none (= abs), 1 abs, 2 shift, 3 saturate */
	int parity_depth;                       /* -P: 0 off; the original's bit depth, 1..16 (lroundf of value * (2^depth - 1)) or 32 (float ==) */
} dspfft_scan_frame_opts;
typedef struct dspfft_scanframes_s *dspfft_scanframes;
/* -s implies -v and -M implies -i, as scan.c:179-186 sets them.  A build without the kernels (the CPU emulation) creates the handle and
 * answers frame_floats; every call that launches reports "not in this build". */
int dspfft_scanframes_create(dspfft_scanframes *sf, uint32_t w, uint32_t h, const dspfft_scan_frame_opts *opts);
/* 3 W' H' */
size_t dspfft_scanframes_frame_floats(dspfft_scanframes sf);
/* clears d_frame, sets the scaler from d_coeffs[0..2] and resets the parity measurement */
int dspfft_scanframes_begin(dspfft_scanframes sf, float *d_frame, const float *d_coeffs, void *hip_stream);
/* lights the top-right panel at every pixel whose owner scan index lies in [lo, hi) (d_owner: an owner-index table in which DC KEEPS its
 * index -- dspfft_scan_owner_index, or a magnitude / file index -- not the fused step's tables, where DC is 0xFFFFFFFF).  current != 0 (the
 * frame being emitted; with -i): the bottom-right panel is first cleared where the previous current call lit it, then lit alike.
 * lo == hi lights nothing (a frame past the scan's limit) but still clears.  No-op without -v. */
int dspfft_scanframes_mark_range(dspfft_scanframes sf, float *d_frame, const float *d_coeffs, const uint32_t *d_owner, uint32_t lo, uint32_t hi,
                                 int current, void *hip_stream);
/* the same from y*w+x lists (dspfft_scan_coords layout; 0xFFFFFFFF slots skipped): box, and `file` orders whose indices share pixels.
 * With current != 0 the list is copied (the next current call clears the bottom-right panel there). */
int dspfft_scanframes_mark_coords(dspfft_scanframes sf, float *d_frame, const float *d_coeffs, const uint32_t *d_lin, uint64_t nslots,
                                  int current, void *hip_stream);
/* one launch per frame (plus -M's two-pass min / max and -P's one-lane flag update): d_sum += d_image when d_image is given (required with
 * -i; NULL without it: the fused step added into d_sum), the top-left and bottom-left panels, d_image back to -0.0f.  -P: compares
 * d_sum with d_original (w h 3 floats, required with parity_depth) until the first frame at parity; `frame` (0-based, i - offset in scan's
 * loop) is what dspfft_scanframes_parity reports. */
int dspfft_scanframes_compose(dspfft_scanframes sf, float *d_frame, float *d_sum, float *d_image, const float *d_coeffs, const float *d_original,
                              uint64_t frame, void *hip_stream);
/* synchronises the stream; *first_frame = the first frame at parity, UINT64_MAX if none was */
int dspfft_scanframes_parity(dspfft_scanframes sf, uint64_t *first_frame, void *hip_stream);
void dspfft_scanframes_destroy(dspfft_scanframes sf);

/* ---- transfer characteristics: scan -g, zoom -g, motion --linear (scan.c:412-414,455-457,486-488, zoom.c:393-399, motion.c:632-633,
 * 768-769) ----
 * The reference takes the functions from libavutil (av_csp_trc_func_from_id and its inverse); the table in dspfun_amd/csrc/trc_core.h is
 * written from the standards and from recollection of libavutil's csp.c (parity unpinned).  Ids are AVColorTransferCharacteristic's, names
 * av_color_transfer_name's.  Built: the ids below; log100, log316, bt1361e, smpte2084, smpte428 and arib-std-b67 are refused.
 * The frame kernels and dspfft_trc_apply_f32 evaluate float -> float within 1 float ulp of the double evaluation rounded to float, bit-equal
 * where that is +-0, NaN or +-inf; motion's load and store evaluate in double as the reference does. */
enum { DSPFFT_TRC_NONE = 0, DSPFFT_TRC_BT709 = 1, DSPFFT_TRC_GAMMA22 = 4, DSPFFT_TRC_GAMMA28 = 5, DSPFFT_TRC_SMPTE170M = 6,
       DSPFFT_TRC_SMPTE240M = 7, DSPFFT_TRC_LINEAR = 8, DSPFFT_TRC_IEC61966_2_4 = 11, DSPFFT_TRC_IEC61966_2_1 = 13,
       DSPFFT_TRC_BT2020_10 = 14, DSPFFT_TRC_BT2020_12 = 15 };
int dspfft_trc_from_name(const char *name);                 /* id, or -1: unknown or not built */
const char *dspfft_trc_name(int trc);                       /* NULL when not built */
/* d_dst[i] = inverse ? decode(d_src[i]) : encode(d_src[i]); d_dst == d_src allowed; the input side of scan -g / zoom -g.  HIP-only. */
int dspfft_trc_apply_f32(float *d_dst, const float *d_src, uint64_t len, int trc, int inverse, void *hip_stream);
/* scan -g: compose encodes what it stores into the top-left and bottom-left panels (scan.c:412-414,455-457,486-488); d_sum, -P and -M
 * stay on linear values, the right-hand panels are never encoded.  0 (the default): frames as without the call, byte for byte. */
int dspfft_scanframes_set_trc(dspfft_scanframes sf, int trc);

/* ---- the rest of motion's block loop (motion/motion.c), HIP-only entry points ---- */
enum { DSPFFT_MOTION_NONE = 0, DSPFFT_MOTION_ABS = 1, DSPFFT_MOTION_SHIFT = 2, DSPFFT_MOTION_FLAT = 3, DSPFFT_MOTION_COPY = 4 };
/* motion.c:617-640: the {n[0],n[1],n[2]} corner of an 8-bit buffer -> float, both laid out as planes of minbuf_hw[0] x minbuf_hw[1];
 * ispec_mode decodes an input spectrogram (--ispec: shift uses ic = 127.5 / log1p(N normalization 255 8), :568,626-628) */
int dspfft_motion_load_u8(float *d_coeffs, const uint8_t *d_pix, const int n[3], const int minbuf_hw[2], int ispec_mode, double ic, double normalization, void *hip_stream);
/* motion.c:756-776: pel = coeff * scalefactor * normalization, then the --spec encode (abs / shift with constant c, :755,762-763; flat :764)
 * or * normalization again (none / copy, :767), clamp and lround to 8 bits */
int dspfft_motion_store_u8(uint8_t *d_pix, const float *d_coeffs, const int n[3], const int minbuf_hw[2], int spec_mode,
                           double scalefactor, double normalization, double c, void *hip_stream);
/* the same two with float pixels (motion's float_pixels: planar float formats): the load reads sample * 255 (motion.c:623), the store writes
 * pel / 255 unclamped (:774) */
int dspfft_motion_load_f32(float *d_coeffs, const float *d_pix, const int n[3], const int minbuf_hw[2], int ispec_mode, double ic, double normalization, void *hip_stream);
int dspfft_motion_store_f32(float *d_pix, const float *d_coeffs, const int n[3], const int minbuf_hw[2], int spec_mode,
                            double scalefactor, double normalization, double c, void *hip_stream);
/* The store and the load of a spectrogram over ALL blocks of a batch in one launch (what dspfft_execute_spectrogram_* and
 * dspfft_execute_ispectrogram_* run beside the passes of a plan that is no small-block plan).  Block b of nblocks lies at b * block_stride
 * elements and its element (z, y, x) at (z minbuf_hw[0] + y) minbuf_hw[1] + x, in d_pix and d_coeffs alike (nblocks = 1: block_stride is
 * not consulted).  The filter acts on the block's own positions inside filter->active; filter == NULL: none.
 *   spec_blocks   d_coeffs is READ, never written: per coefficient the filter (motion.c:683-744), then the encode with sp (:755-771; abs:
 *                 c from the block's element 0 as d_coeffs holds it, :650,755) and the store (:774,776).  5 B/sample on 8-bit pixels.
 *   ispec_blocks  per pixel the load (:621-625), the decode with sp (:627-630; sp->c is ic) and the filter, into d_coeffs.
 * sp->mode none is allowed in both (the plain load and store); abs in spec_blocks only.  Errors: dspfft_motion_last_error. */
int dspfft_motion_spec_blocks_u8(uint8_t *d_pix, const float *d_coeffs, const int n[3], const int minbuf_hw[2], size_t nblocks, long long block_stride,
                                 const dspfft_motion_spec_params *sp, const dspfft_motion_filter_params *filter, unsigned long long *d_coeffs_coded, void *hip_stream);
int dspfft_motion_spec_blocks_f32(float *d_pix, const float *d_coeffs, const int n[3], const int minbuf_hw[2], size_t nblocks, long long block_stride,
                                  const dspfft_motion_spec_params *sp, const dspfft_motion_filter_params *filter, unsigned long long *d_coeffs_coded, void *hip_stream);
int dspfft_motion_ispec_blocks_u8(float *d_coeffs, const uint8_t *d_pix, const int n[3], const int minbuf_hw[2], size_t nblocks, long long block_stride,
                                  const dspfft_motion_spec_params *sp, const dspfft_motion_filter_params *filter, unsigned long long *d_coeffs_coded, void *hip_stream);
int dspfft_motion_ispec_blocks_f32(float *d_coeffs, const float *d_pix, const int n[3], const int minbuf_hw[2], size_t nblocks, long long block_stride,
                                   const dspfft_motion_spec_params *sp, const dspfft_motion_filter_params *filter, unsigned long long *d_coeffs_coded, void *hip_stream);
/* The 8-bit pair on PACKED pixels, over `frames` dense frames [h][w][components] that d_pix and d_coeffs share element for element (what
 * dspfft_execute_spectrogram_u8_packed / _ispectrogram_u8_packed run beside the passes of a full-frame plan; motion_spec_packed.hip).  Every
 * component of a frame is a block of its own: element e of a row belongs to component e mod components at x = e / components, abs takes a
 * component's c from that component's DC at the frame's first pixel, and packed->damp, boost and grey_add (by byte position) replace the
 * filter's.  A thread moves one dword of pixels and a float4 of coefficients where w * components is a multiple of 4, d_pix 4-byte and
 * d_coeffs 16-byte aligned, one sample otherwise.  The bytes (coefficients) EQUAL those of the planar pair on each de-interleaved component
 * with n = (1, h, w) and nblocks = frames.  sp->mode none is allowed in both, abs in spec_blocks only; components must be 2, 3 or 4 and
 * equal packed->components.  Errors: dspfft_motion_last_error. */
int dspfft_motion_spec_blocks_u8_packed(uint8_t *d_pix, const float *d_coeffs, int h, int w, int components, size_t frames, const dspfft_motion_spec_params *sp,
                                        const dspfft_motion_filter_params *filter, const dspfft_motion_packed *packed, unsigned long long *d_coeffs_coded, void *hip_stream);
int dspfft_motion_ispec_blocks_u8_packed(float *d_coeffs, const uint8_t *d_pix, int h, int w, int components, size_t frames, const dspfft_motion_spec_params *sp,
                                         const dspfft_motion_filter_params *filter, const dspfft_motion_packed *packed, unsigned long long *d_coeffs_coded, void *hip_stream);
/* motion's coefficient filter (motion.c:683-744; dspfft_motion_filter below is the planar form) over `frames` dense frames [h][w][components]
 * of coefficients in d_coeffs, in place: the middle step of dspfft_execute_roundtrip_u8_packed_frames where its column passes run unfused
 * (motion_filter_packed.hip).  Every component of a frame is a block of its own: element e of a frame lies in row e / (w components), at pixel
 * x = (e mod (w components)) / components, in component e mod components, and goes through the filter at (0, y, x) with that component's
 * packed->damp, boost and grey_add (by byte position; the filter's fields of those names are not read).  filter->active = (d, h', w') in
 * pixels: pixels outside it stay as they are; minbuf_hw and block_depth are checked, not read.  A thread moves a float4 where w * components is
 * a multiple of 4 and d_coeffs 16-byte aligned, one coefficient otherwise; frames go along the grid's y, so offsets stay frame-local (a frame
 * of 2^32 samples or more is refused); d_coeffs_coded takes one atomic per wave.  The coefficients EQUAL those of dspfft_motion_filter on each
 * de-interleaved component with that component's damp, boost and grey_add, the count their sum.  components must be 2, 3 or 4 and equal
 * packed->components.  Errors: dspfft_motion_last_error. */
int dspfft_motion_filter_packed(float *d_coeffs, int h, int w, int components, size_t frames, const dspfft_motion_filter_params *filter,
                                const dspfft_motion_packed *packed, unsigned long long *d_coeffs_coded, void *hip_stream);
/* the float-pixel pair with motion --linear, which the reference applies with --ispec / --spec none (and copy on the store) only:
 * load  pel = sample * 255 (a float product); coeff = (float)(decode(pel / 255) * 255)          (motion.c:623,633)
 * store pel = coeff * scalefactor * normalization; pel *= normalization; sample = (float)(encode(pel / 255) * 255 / 255)   (:759,767-769,774)
 * in double with the exact evaluation.  -1 for a trc that is 0 or not built. */
int dspfft_motion_load_f32_linear(float *d_coeffs, const float *d_pix, const int n[3], const int minbuf_hw[2], int trc, void *hip_stream);
int dspfft_motion_store_f32_linear(float *d_pix, const float *d_coeffs, const int n[3], const int minbuf_hw[2],
                                   double scalefactor, double normalization, int trc, void *hip_stream);
/* the 8-bit pair with motion --linear (--ispec / --spec none; a copy store alike), through the two tables of dspfft_plan_set_u8_trc:
 * load  coeff = lut[byte] = (float)(decode(byte / 255) * 255) as the reference's default (long double) build stores it      (motion.c:625,633,637)
 * store pel = coeff * scalefactor * normalization; pel *= normalization (double); byte = clamp(lround(encode(pel / 255) * 255))   (:759,767-769,776)
 * -1 for a trc that is 0 or not built.  The tables of these calls (and of the flat pair and the dithered store below) are uploaded once per
 * device and function, synchronously at the first call that needs them, and kept for the life of the process. */
int dspfft_motion_load_u8_linear(float *d_coeffs, const uint8_t *d_pix, const int n[3], const int minbuf_hw[2], int trc, void *hip_stream);
int dspfft_motion_store_u8_linear(uint8_t *d_pix, const float *d_coeffs, const int n[3], const int minbuf_hw[2],
                                  double scalefactor, double normalization, int trc, void *hip_stream);
/* motion.c:756-788 with -d / --dither (spec none, 8-bit pixels, !linear): the 8-bit store with 2-D Floyd-Steinberg error diffusion, plane
 * by plane (the z planes of a block are independent, and so are blocks).  Per pixel, in raster order: pel = c * scalefactor * normalization,
 * pel *= normalization, byte = clamp + lround, dp = c - byte / (normalization^2 scalefactor), and dp * 7/16, 3/16, 5/16, 1/16 go into the
 * right, lower-left, lower and lower-right neighbours, each `+=` rounding to float -- so the order in which a pixel receives them (1/16, 5/16,
 * 3/16 from the row above, then 7/16 from the left) is part of the result and is kept.
 * Element (block b0,b1,b2; plane z; row y; column x) is at b0 block_step[0] + b1 block_step[1] + b2 block_step[2] + z plane_pitch +
 * y row_pitch + x, in d_pix and d_coeffs alike.  Covers a stack of frames (per-frame blocks: n = {1,h,w}, nblocks = {frames,1,1}), one 3-D
 * block (n = {d,h,w}), small blocks as a block-major stack or lying in a volume (one nblocks / block_step per axis).
 * d_coeffs is READ, never written (the reference diffuses into its coefficient buffer, which nothing reads afterwards).
 * Precision: intermediates in double, in the reference's operation order, nothing contracted into an FMA: byte-identical to the reference's
 * lines built with COEFF_PRECISION=F INTERMEDIATE_PRECISION=D.  Against the tool's default long double build (=L) the bytes CANNOT match in
 * general: error diffusion is chaotic, one last-bit difference flips a rounding and the pattern downstream follows -- +-1 on some per cent of
 * the pixels of a whole frame, 8x8 block means within 0.1 (tests/test_motion_dither_cpu.py pins both bars).
 * Planes up to 64 wide and 1024 samples run one lane per plane; larger ones a wavefront over a workgroup (rows up to about 9000 samples). */
typedef struct {
	int n[3];                               /* scaled block extent {d, h, w}; dithered plane by plane */
	long long row_pitch, plane_pitch;       /* elements, shared by d_pix and d_coeffs */
	int nblocks[3];                         /* blocks along {d, h, w} (any three batch axes); {1,1,1} for one block */
	long long block_step[3];                /* elements between neighbouring blocks along each of them */
} dspfft_dither_geom;
int dspfft_motion_dither_u8(uint8_t *d_pix, const float *d_coeffs, const dspfft_dither_geom *g, double scalefactor, double normalization, void *hip_stream);
/* the same with motion --linear: the byte is clamp(lround(encode(pel / 255) * 255)) (:769,776), found in the threshold table of
 * dspfft_plan_set_u8_trc; the error is still c - byte / (normalization^2 scalefactor) (:780: the reference subtracts an encoded byte from a
 * linear coefficient, and so does this).  Byte-identical to the reference's lines built F / D with linear = true.  -1 for a trc that is 0 or
 * not built. */
int dspfft_motion_dither_u8_trc(uint8_t *d_pix, const float *d_coeffs, const dspfft_dither_geom *g, double scalefactor, double normalization, int trc, void *hip_stream);
/* The two calls above on PACKED pixels: d_pix and d_coeffs hold `components` (2, 3 or 4) values per pixel, every component of a pixel plane is
 * a plane of its own (motion.c:613-615), and there are `components` times as many planes.  g is in PIXELS exactly as above: the element of
 * component c is at components * (the pixel offset above) + c.  The same two kernels with an element step, the regime chosen from the plane's
 * extent in pixels as above.  trc = 0: the plain byte; else the encoded one (dspfft_motion_dither_u8_trc).  -1 for components outside 2..4 and
 * for everything the planar call refuses; -3 from a library built without the HIP kernels; the reason in dspfft_last_error. */
int dspfft_motion_dither_u8_packed(uint8_t *d_pix, const float *d_coeffs, const dspfft_dither_geom *g, int components, double scalefactor, double normalization,
                                   int trc /* 0: plain */, void *hip_stream);
/* motion.c:652-668 (--coeff-limit): keep the `keep` coefficients of largest magnitude among d_coeffs[0 .. count), zero the rest.
 * Radix select on the device (four histogram passes over the bits of |c|, no sort).  Ties at the threshold: the reference's choice
 * depends on qsort; here the earliest in buffer order are kept -- documented, deterministic. */
size_t dspfft_motion_topn_work_bytes(size_t count);
int dspfft_motion_topn(float *d_coeffs, size_t count, size_t keep, void *d_work, size_t work_bytes, void *hip_stream);
/* The same selection in each of `nblocks` contiguous runs of `count` floats, `block_stride` floats apart (>= count): a block-major stack of
 * blocks, the frames of a clip, one 3-D block (motion --coeff-limit with -b 8x8x8, -b 0x0x1, one block).  keep == 0 zeroes every run, keep >=
 * count is a no-op; what lies between the runs is never touched.  Runs of up to 4096 floats are selected in LDS, a wave per run, by the code
 * the fused block roundtrip runs (topn_core.h: 31 ballot rounds over the bits of |c|), and need no work buffer (d_work may be NULL, the byte
 * count is 0); longer ones take the radix select above with one histogram per run, as many runs per launch as 2^26 elements' worth.
 * The reference selects over `mincomponent`, the largest component's buffer: a run is the block's own embedding. */
size_t dspfft_motion_topn_blocks_work_bytes(size_t count, size_t nblocks);
int dspfft_motion_topn_blocks(float *d_coeffs, size_t count, size_t nblocks, long long block_stride, size_t keep, void *d_work, size_t work_bytes,
                              void *hip_stream);
const char *dspfft_motion_last_error(void);

/* ---- rotate (motion/rotate.c): a clip's three axes permuted, with flips ---- */

/* rotate.c:74-89 on `spec` ("zyx", "-yx+z", ...), host only: at position p a '-' sets invert[p] and a '+' is skipped, each before the letter
 * of its own position, and the letter gives map[p] = letter - 'x'; what follows the third letter is not read.  Non-zero for a string the
 * reference sends to usage() and, beyond the reference, for a map that is no permutation ("xxy"). */
int dspfft_rotate_parse(const char *spec, int map[3], int invert[3]);
/* rotate.c:159-164 on a dense device clip d_in[len[2]][len[1]][len[0]] of elements of elem_bytes = 1 (a planar 8-bit plane), 2, 3 (rgb24),
 * 4 (rgba, or a planar float plane): output axis o (0 = x) runs over input axis map[o], so d_out is [len[map[2]]][len[map[1]]][len[map[0]]],
 * and input axis a is read backwards iff invert[map[a]] -- for the two 3-cycles not the axis the signed letter names ("-yzx" flips input z),
 * as the reference.  Stream-ordered, no allocation, no host synchronisation; all offsets 64-bit.  The base pointers need only be aligned to
 * the element (2 and 4 bytes: to that many; 1 and 3: any address), so -s start:nframes is d_in + start len[0] len[1] elem_bytes and a
 * smaller len[2].  Non-zero, with the reason in dspfft_motion_last_error() and nothing launched: a zero extent, elem_bytes outside 1..4, a
 * map that is no permutation, a null or misaligned pointer, overlapping input and output (there is no in-place form), more than 2^31 - 1
 * tiles. */
int dspfft_rotate(void *d_out, const void *d_in, const uint64_t len[3], int elem_bytes, const int map[3], const int invert[3], void *hip_stream);

/* scan/scan.c:451-459 arithmetic: sum += image (len floats). */
int dspfft_accumulate(float *d_sum, const float *d_image, uint64_t len, void *hip_stream);

/* scan/scan.c:377-383: sum[p*channels + z] = coeffs[z] for every pixel p. */
int dspfft_broadcast_dc(float *d_sum, const float *d_coeffs, uint64_t npixels, int channels, void *hip_stream);

/* motion/motion.c:617-638 (ispec none, !linear, 8-bit input): coeffs[i] = (float)pix[i]. */
int dspfft_u8_to_f32(float *d_dst, const uint8_t *d_src, uint64_t len, void *hip_stream);

/* motion/motion.c:756-776 (spec none, !linear, 8-bit output): pix = clamp(lround(c * mul), 0, 255). */
int dspfft_f32_to_u8(uint8_t *d_dst, const float *d_src, double mul, uint64_t len, void *hip_stream);

/* the same two with motion --linear (motion.c:633, :769): dst = lut[src], and dst = the byte of the linear value (double)src * mul, by the
 * tables of dspfft_plan_set_u8_trc.  Any alignment; 4-byte aligned bytes beside 16-byte aligned floats move four samples per lane.
 * -1 for a trc that is 0 or not built. */
int dspfft_u8_to_f32_trc(float *d_dst, const uint8_t *d_src, uint64_t len, int trc, void *hip_stream);
int dspfft_f32_to_u8_trc(uint8_t *d_dst, const float *d_src, double mul, uint64_t len, int trc, void *hip_stream);

/* ---- zoom's dense basis product on the f32 matrix cores ---- */

/* zoom/zoom.c:37-41: number of cosine components kept for a (scale, length) pair. */
size_t dspfft_zoom_ncomponents(double scale_num, double scale_den, size_t len);

/* zoom/zoom.c:36-68 (generate_scaled_basis): d_basis[b*nc + n], nc = dspfft_zoom_ncomponents(...), with
 * column 0 = 1/2 (the halved DC term of zoom.c:364,369) and column n >= 1 = cos(pi (k+1/2) n / N).
 * type: 0 interpolated, 1 centered, 2 native (zoom/zoom.c:20-26). */
int dspfft_zoom_basis(float *d_basis, int type, double scale_num, double scale_den, double offset,
                      size_t nvectors, size_t len, void *hip_stream);

/* zoom/zoom.c:361-375: out (vh x vw x 3) = YB . (C_z[:ch,:cw] . XB^T) / (w h) for the three channels of the
 * unnormalised REDFT10^2 coefficients d_coeffs (h x w x 3 interleaved).  d_work: dspfft_zoom_work_floats(). */
size_t dspfft_zoom_work_floats(int w, int h, size_t ch, int vw);
int dspfft_zoom_product(const float *d_coeffs, int w, int h, const float *d_xb, size_t cw, const float *d_yb, size_t ch,
                        float *d_out, int vw, int vh, float *d_work, void *hip_stream);

/* The GEMM underneath (also the building block for applybasis' basis x pixel sums):
 * C[m*ldc + n*cs] = alpha * sum_k A[m*lda + k] * B[n*ldb + k], `batch` problems at offsets sa/sb/sc. */
int dspfft_gemm_nt_f32(const float *A, const float *B, float *C, int M, int N, int K,
                       long long lda, long long ldb, long long ldc, int cs,
                       int batch, long long sa, long long sb, long long sc, float alpha, void *hip_stream);
const char *dspfft_zoom_last_error(void);

/* The same frame by fast transforms, for the scales at which an axis's output samples lie on a DCT-III grid: `interpolated` (0) or
 * `native` (2) basis with len * num / den an integer M on both axes and a viewport of at most Mx x My samples (any offset: a pan
 * re-plans nothing).  Per axis  out[b] = 1/2 REDFT01_M(C[n] cos(theta n))[b] - (-1)^b 1/2 REDFT01_M(C[M - n'] sin(theta (M - n')))[b],
 * theta = pi (offset + (s - 1) / 2) / M (interpolated), pi offset / M (native)  (zoom/zoom.c:49-57): two
 * length-M REDFT01 executions per axis on the row / column kernels instead of the dense product -- BASELINE config 3 (4x of
 * 1920x1080): 310 GFLOP become about 1 GB of streaming in three transform launches.  dspfft_zoomfft_create returns -2 when the scale,
 * basis or viewport does not qualify (use dspfft_zoom_product then); d_coeffs, d_out (vh x vw x 3) and d_work
 * (dspfft_zoomfft_work_floats floats) 16-byte aligned.  One object serves one stream at a time. */
typedef struct dspfft_zoomfft_s *dspfft_zoomfft;
int dspfft_zoomfft_create(dspfft_zoomfft *z, int w, int h, int type, double xscale_num, double xscale_den, double yscale_num, double yscale_den,
                          int vw, int vh);
size_t dspfft_zoomfft_work_floats(dspfft_zoomfft z);
int dspfft_zoomfft_execute(dspfft_zoomfft z, const float *d_coeffs, double vx, double vy, float *d_out, float *d_work, void *hip_stream);
void dspfft_zoomfft_destroy(dspfft_zoomfft z);
const char *dspfft_zoomfft_last_error(void);
/* zoom's frame at ANY scale, offset and basis (interpolated, centered, native) by chirp-z transforms along both axes: same arguments as
 * dspfft_zoomfft_*, no restriction on the scaled lengths (dspfft_zoomfft_* needs them integer and refuses `centered`).  -2 when an axis is
 * longer than the longest listed convolution (coefficients + samples - 1 > 19200): the dense product (dspfft_zoom_product) remains. */
typedef struct dspfft_zoomczt_s *dspfft_zoomczt;
int dspfft_zoomczt_create(dspfft_zoomczt *z, int w, int h, int type, double xnum, double xden, double ynum, double yden, int vw, int vh);
size_t dspfft_zoomczt_work_floats(dspfft_zoomczt z);
int dspfft_zoomczt_execute(dspfft_zoomczt z, const float *d_coeffs, double vx, double vy, float *d_out, float *d_work, void *hip_stream);
void dspfft_zoomczt_destroy(dspfft_zoomczt z);
/* zoom's animation loop (zoom/zoom.c:320-410): one object per geometry (w, h, basis type, vw, vh), any scale and offset per frame.
 * create plans the chirp-z rows of dspfft_zoomczt_* once for the largest extents a frame can need (x: nc = w over vh 3 lines; y: nc = h
 * over w 3 lines); -2 when w + vw - 1 or h + vh - 1 exceeds the longest listed convolution (19200) -- keep the dense product then.
 * set_coeffs transposes the h x w x 3 REDFT10^2 block once into the object; call it again whenever the buffer's contents change.
 * execute renders one frame at xscale = xnum / xden, yscale = ynum / yden, offset (vx, vy), with zoom.c:37-41's clamp and component count
 * per axis (a frame below 1x runs on the first cw 3 lines of ch components): no device allocation, no host synchronisation, no re-planning
 * (the chirp spectrum of an axis is rebuilt only when its omega changes).  Always chirp-z: a pan at a fixed integer scale could take
 * dspfft_zoomfft_*, whose offset is per call too.
 *   showsamples  0 none, 1 point, 2 grid: zoom.c:377-390 when xscale > 1 && yscale > 1 -- (0, 1, 0) at the linear index y vh + x of the
 *                frame (vh, not vw, as the reference); with vh > vw the reference writes past its frame and indices >= vw vh are dropped
 *                here; negative offsets (undefined there) go through long long (zoom_anim_core.h).
 *   layout       0 interleaved RGB (vh x vw x 3), 1 GBRPF32 (three vw x vh planes G, B, R: libavutil's comp[] order).
 * A finite scale with len num / den < 1 -- zero and negative numerators included -- is clamped to 1 / len as zoom.c:37-41 does: one
 * component, a frame of the DC term alone (the reference itself then asks realloc for 0 bytes of basis, zoom.c:42, and may crash).
 * Returns -2 (nothing written) for a degenerate `centered` frame (len num - den <= 0 after the clamp), -1 for a non-finite scale or
 * offset or a denominator <= 0 (the caller skips non-finite frames, zoom.c:342-345), -3 for any showsamples != 0 or layout 1 in a build
 * without the kernels (the CPU emulation), whether or not the overlay would apply to the frame.
 * d_out and d_work (dspfft_zoomanim_work_floats floats) 16-byte aligned; one object serves one stream at a time. */
typedef struct dspfft_zoomanim_s *dspfft_zoomanim;
int dspfft_zoomanim_create(dspfft_zoomanim *z, int w, int h, int type, int vw, int vh);
size_t dspfft_zoomanim_work_floats(dspfft_zoomanim z);
int dspfft_zoomanim_set_coeffs(dspfft_zoomanim z, const float *d_coeffs, void *hip_stream);
int dspfft_zoomanim_execute(dspfft_zoomanim z, double xnum, double xden, double ynum, double yden, double vx, double vy,
                            int showsamples, int layout, float *d_out, float *d_work, void *hip_stream);
void dspfft_zoomanim_destroy(dspfft_zoomanim z);
const char *dspfft_zoomanim_last_error(void);
/* zoom -g: every output sample is encoded after the overlay (zoom.c:377-399; the green marker goes through it like any sample), in place
 * on the interleaved frame and inside the planar store.  0 (the default): launches and bytes as without the call.  A trc other than 0
 * makes dspfft_zoomanim_execute return -3 in a build without the kernels. */
int dspfft_zoomanim_set_trc(dspfft_zoomanim z, int trc);

/* ---- applybasis' basis x pixel partial sums on the matrix cores ----
 * applybasis/applybasis.c:410-431, forward direction:
 *   out[k_h][k_w][n_h][n_w][j] = sum_{s_h < Ph, s_w < Pw} f(k_h + offh, n_h Ph + s_h, h) f(k_w + offw, n_w Pw + s_w, w) pix[..][j]
 * func: 0 dft, 1 idft, 2..5 dct1-4, 6..9 dst1-4, 10 wht, 11 dht (applybasis.c:77-140); d_pixels: h x w x 3 f32 already
 * range-mapped (applybasis.c:358-360); d_out: Kh*Kw*(h/Ph)*(w/Pw)*3 complex (re, im) floats in the order of the tool's
 * `.coeff` dump (applybasis.c:443).  d_work: dspfft_applybasis_work_floats() floats. */
size_t dspfft_applybasis_work_floats(int w, int h, int Kw, int Kh, int Pw, int Ph, int func);
int dspfft_applybasis_partsums(float *d_out, const float *d_pixels, int w, int h, int func, int ortho,
                               int Kw, int Kh, int Pw, int Ph, long long offw, long long offh,
                               float *d_work, void *hip_stream);

/* The general form: N partial-sum blocks of P pixels per axis chosen freely (N x P <= image), real or complex pixels.
 *   forward  (applybasis.c:378-389 with !inverse):  K = terms,       N = image size / partsum
 *   --inverse                                    :  K = image size,  N = terms / partsum
 *   .coeff input (applybasis.c:319-338): complex pixels -- d_pix_im non-NULL (planes h x w x 3, like d_pix_re)
 * --offset (applybasis.c:416-420 adds it to `bi`): inverse = 0 -> f(k + off, n P + s); inverse = 1 (`n = &bi`, :372-378) ->
 * f(k, (n + off) P + s) while the pixel read stays at n P + s.
 * Each call is two batched GEMM launches (three basis / layout kernels around them), whatever the function. */
size_t dspfft_applybasis_work_floats_ex(int w, int h, int Kw, int Kh, int Nw, int Nh, int func);
int dspfft_applybasis_partsums_ex(float *d_out, const float *d_pix_re, const float *d_pix_im, int w, int h, int func, int ortho,
                                  int Kw, int Kh, int Nw, int Nh, int Pw, int Ph, long long offw, long long offh, int inverse,
                                  float *d_work, void *hip_stream);
/* applybasis.c:392-442: the rendered frame from the partial sums.  d_frame: fh x fw x 4 floats (RGBA) with
 * fw = Kw Nw scale + padding T_w + padding (T = K forward, N with --inverse), same for fh; filled with padcolor first.
 * plane: 0 real 1 imaginary 2 magnitude 3 phase (:20-31); rescale0 / rescale1: 0 linear 1 log 2 gain 3 level, rescale1 = -1 for a
 * single type, else the two are interpolated as :433-438 does; range: 0 shift / shift2, 1 abs, 2 invert, 3 hue (:46-76);
 * coeff_scale as :399-407; insize_wh = input width x height. */
int dspfft_applybasis_render(float *d_frame, const float *d_partsums, int Kw, int Kh, int Nw, int Nh, int inverse, int scale, int padding,
                             int plane, int rescale0, int rescale1, int range, double coeff_scale, double insize_wh,
                             const float padcolor[4], void *hip_stream);

/* ---- elementwise stages either side of the transform, on the device ---- */

/* spec/spec.c:81-139 on uniform-range coefficients (after the fused normalisation): f *= gain; divisor per channel
 * from rangetype (0 one, 1 dc, 2 dcs; spec.c:92-110); scaletype 0 log (copysign(log1p|f|)/log1p(max), :113-118) or
 * 1 linear (:120-122); signtype 0 abs, 1 shift, 2 saturate, 3 retain (:124-139).  `gain` is the resolved multiplier
 * (native 127.5*sqrt(4wh), reference 127.5*1024, or custom; spec.c:82-87). */
int dspfft_spec_encode(float *d_f, size_t npixels, int channels, double gain, int rangetype, int scaletype, int signtype, void *hip_stream);

/* spec/ispec.c:100-151, the inverse (the separate sign-map image of :91-99 is not handled).  dc: `channels` doubles
 * from the spectrogram's "DC" property (host memory; needed for rangetype dc/dcs and for restore_dc, ispec.c:161-163). */
int dspfft_ispec_decode(float *d_f, size_t npixels, int channels, double gain, int rangetype, int scaletype, int signtype,
                        const double *dc, int restore_dc, void *hip_stream);
/* spec/ispec.c:91-99, run BEFORE dspfft_ispec_decode of an `abs` spectrogram that comes with a sign-map image (-m): every sample but
 * the first pixel's takes the sign of (map - 128); the first pixel of the map carries the DC terms instead (DC[z] = map[z] / 255,
 * host arithmetic on channels bytes -- pass them to dspfft_ispec_decode as `dc`). */
int dspfft_ispec_signmap(float *d_f, const uint8_t *d_map, size_t npixels, int channels, void *hip_stream);

/* motion/motion.c:683-744 on one block of uniform-range coefficients embedded in {., minbuf_h, minbuf_w}: damp outside /
 * boost inside the band-pass box [band_begin, band_end), threshold on |c| (threshold_hi <= 0 disables; bounds already scaled
 * as motion.c:571-572), DC preservation (0 none, 1 dc, 2 grey with grey_add = (1 - (dcstop ? damp : boost)) * 127.5 /
 * (normalization^2 * scalefactor), :736), quantisation round(c/Q)*Q (Q <= 0 disables).  d_coeffs_coded (optional, device)
 * accumulates the count of non-zero quantised coefficients (:744).  All index triples are {d, h, w}. */
int dspfft_motion_filter(float *d_coeffs, const int active[3], const int minbuf_hw[2], const int band_begin[3], const int band_end[3],
                         float damp, float boost, float threshold_lo, float threshold_hi, int preserve_dc, float grey_add,
                         float quantizer, unsigned long long *d_coeffs_coded, void *hip_stream);
/* scan/scan.c:20-41,449 (pruned_idct) fused with the accumulate of :451-459:
 *   sum[y][x][z] += sum_n coeffs[lin[n]][z] * B_h[y][cy_n] * B_w[x][cx_n],  B_N[k][j] = j ? 2 cos(pi j (k+1/2)/N) : 1
 * for the `ncoords` coefficients (device list of y*w+x offsets) one output frame adds.  The reference takes this path
 * when step * max_interval <= log2(w*h) (scan.c:349-350).  The caller leaves the DC pixel out of the list (scan.c:445). */
int dspfft_scan_pruned_accumulate(float *d_sum, const float *d_coeffs, const uint32_t *d_lin, int ncoords,
                                  int w, int h, int channels, void *hip_stream);
/* the same with its basis table in a caller-provided buffer of dspfft_scan_pruned_work_floats(ncoords, w, h) floats: no allocation
 * inside the call, so a scan loop on the pruned path can be captured into a hipGraph (dspfft_scan_pruned_accumulate allocates per call) */
size_t dspfft_scan_pruned_work_floats(int ncoords, int w, int h);
int dspfft_scan_pruned_accumulate_ws(float *d_sum, const float *d_coeffs, const uint32_t *d_lin, int ncoords,
                                     int w, int h, int channels, float *d_work, void *hip_stream);
const char *dspfft_pointwise_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
