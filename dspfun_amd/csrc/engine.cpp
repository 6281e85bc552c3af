// engine.cpp -- plan construction and execution behind include/dspfft.h.
//
// Mirrors the contract of the FFTW calls the reference makes through `fftw(call)`
// (reference include/precision.h:115): plan_many_r2r captures geometry (spec/spec.c:63,
// spec/ispec.c:165, zoom/zoom.c:263, scan/scan.c:292,359, motion/motion.c:535-552), execute runs
// it any number of times (scan/scan.c:447 runs one plan per output frame).  A plan is a list of
// 1-D axis passes over device memory; each pass is one kernel launch (see dct_core.h).
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <complex>
#include <mutex>
#include <dlfcn.h>
#include <memory>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/dspfft.h"
#include "backend.h"
#include "scan_frame_core.h"
#include "zoom_anim_core.h"
#include "trc_core.h"
#include "topn_core.h"
#include "block_rt.h"
#include "block_rs_core.h"
#include "block_packed_core.h"
#include "block_rs_packed_core.h"
#include "block_rs_packed_wide_core.h"
#include "temporal_core.h"
#include "block_spec_core.h"
#include "block_spec_packed_core.h"
#include "trc_u8_core.h"
#include "spec_image_core.h"
#include "dct_spec.h"
#include "spec_list.h"

using namespace dspfft;

// motion_dither.hip's launcher (dspfft_motion_dither_u8's body).  Weak: the CPU emulation build of this file has no HIP kernels, the
// reference is then null and the dithered roundtrip reports that it is not in the build.
extern "C" __attribute__((weak, visibility("hidden"))) int dspfft_dither_launch(uint8_t *d_pix, const float *d_coeffs, const dspfft_dither_geom *g,
                                                                                 double scalefactor, double normalization, void *stream, char *err, size_t errlen);

// scan_frame.hip's launcher (the dspfft_scanframes_* bodies).  Weak, as dspfft_dither_launch: the CPU emulation build reports "not in this build".
extern "C" __attribute__((weak, visibility("hidden"))) int dspfft_scanframes_launch(dspfft::SfOp *o, char *err, size_t errlen);
// zoom_anim.hip's launcher (the overlay and planar store of dspfft_zoomanim_execute).  Weak, as above.
extern "C" __attribute__((weak, visibility("hidden"))) int dspfft_zoomanim_finish_launch(float *d_out, const float *src, const dspfft::ZaOverlay *o,
                                                                                          int planar, int trc, void *stream, char *err, size_t errlen);
// pointwise.hip's and motion_ops.hip's launchers behind dspfft_trc_apply_f32 and dspfft_motion_{load,store}_f32_linear.  Weak, as above.
extern "C" __attribute__((weak, visibility("hidden"))) int dspfft_trc_apply_launch(float *d_dst, const float *d_src, uint64_t len, int trc, int inverse, void *stream);
extern "C" __attribute__((weak, visibility("hidden"))) int dspfft_motion_linear_launch(float *d_dst, const float *d_src, const int n[3], const int minbuf_hw[2], int store,
                                                                                        double scalefactor, double normalization, int trc, void *stream);

// block_topn.hip's and motion_ops.hip's launchers behind dspfft_execute_roundtrip_topn / _u8_topn.  Weak, as above.
extern "C" __attribute__((weak, visibility("hidden"))) int dspfft_block_topn_launch(const dspfft::BlockRtTopnArgs *a, int nwg, size_t lds, void *stream);
extern "C" __attribute__((weak, visibility("hidden"))) int dspfft_topn_blocks_launch(float *d_coeffs, size_t count, size_t nblocks, long long block_stride, size_t keep,
                                                                                      void *d_work, size_t work_bytes, int restore_dc, void *stream);
extern "C" __attribute__((weak, visibility("hidden"))) size_t dspfft_topn_blocks_bytes(size_t count, size_t nblocks);
extern "C" __attribute__((weak)) const char *dspfft_motion_last_error(void);
// motion --linear on 8-bit samples (dspfft_plan_set_u8_trc and the stand-alone calls): motion_ops.hip's flat and region kernels,
// motion_dither.hip's dithered store, block_trc.hip's fused block roundtrip and spec_inst_row_trc.hip's row ends.  Weak, as above.
extern "C" __attribute__((weak, visibility("hidden"))) int dspfft_u8_trc_flat_launch(void *d_dst, const void *d_src, double mul, uint64_t len, int store, int trc, const void *tab, void *stream);
extern "C" __attribute__((weak, visibility("hidden"))) int dspfft_u8_trc_region_launch(void *d_dst, const void *d_src, const int n[3], const long long sdst[3], const long long ssrc[3], int store,
                                                                                        double m0, double m1, double m2, int trc, const void *tab, void *stream);
extern "C" __attribute__((weak, visibility("hidden"))) int dspfft_dither_trc_launch(uint8_t *d_pix, const float *d_coeffs, const dspfft_dither_geom *g, double scalefactor,
                                                                                     double normalization, int trc, const void *tab, void *stream, char *err, size_t errlen);
extern "C" __attribute__((weak, visibility("hidden"))) int dspfft_block_trc_launch(const dspfft::BlockRtTrcArgs *a, int nwg, size_t lds, void *stream);
// block_rescale.hip's launcher behind a roundtrip over a rescaled block grid (motion -b with -s).  Weak, as above.
extern "C" __attribute__((weak, visibility("hidden"))) int dspfft_block_rescale_launch(const dspfft::BlockRsArgs *a, int nwg, size_t lds, void *stream);
// block_rescale_topn.hip's launcher behind the same with a coefficient limit (dspfft_execute_roundtrip_limit and its kin).  Weak, as above.
extern "C" __attribute__((weak, visibility("hidden"))) int dspfft_block_rescale_topn_launch(const dspfft::BlockRsTopnArgs *a, int nwg, size_t lds, void *stream);
// block_packed.hip's launcher behind dspfft_execute_roundtrip_u8_packed (packed 8-bit pixels through the fused block roundtrip).  Weak, as above.
extern "C" __attribute__((weak, visibility("hidden"))) int dspfft_block_rescale_packed_launch(const dspfft::BlockRsPackedArgs *a, int nwg, size_t lds, void *stream);
// block_rescale_packed_limit.hip's and block_rescale_packed_dither.hip's launchers behind dspfft_execute_roundtrip_u8_packed_rescale_limit / _dither.  Weak, as above.
extern "C" __attribute__((weak, visibility("hidden"))) int dspfft_block_rescale_packed_limit_launch(const dspfft::BlockRsPackedWideArgs *a, int nwg, size_t lds, void *stream);
extern "C" __attribute__((weak, visibility("hidden"))) int dspfft_block_rescale_packed_dither_launch(const dspfft::BlockRsPackedWideArgs *a, int nwg, size_t lds, void *stream);
extern "C" __attribute__((weak, visibility("hidden"))) int dspfft_block_packed_launch(const dspfft::BlockPackedArgs *a, int nwg, size_t lds, void *stream);
// block_packed_dither.hip's launcher behind dspfft_execute_roundtrip_u8_packed_dither, and motion_dither.hip's behind dspfft_motion_dither_u8_packed
// (dry: its checks alone).  Weak, as above.
extern "C" __attribute__((weak, visibility("hidden"))) int dspfft_block_packed_dither_launch(const dspfft::BlockPackedDitherArgs *a, int nwg, size_t lds, void *stream);
extern "C" __attribute__((weak, visibility("hidden"))) int dspfft_dither_packed_launch(uint8_t *d_pix, const float *d_coeffs, const dspfft_dither_geom *g, int comps, double scalefactor,
                                                                                       double normalization, int trc, const void *tab, int dry, void *stream, char *err, size_t errlen);
// temporal_rt.hip's launcher behind a roundtrip over blocks along time (motion -b 1x1xD).  Weak, as above.
extern "C" __attribute__((weak, visibility("hidden"))) int dspfft_temporal_rt_launch(const dspfft::TemporalArgs *a, int nwg, void *stream);
// block_spec.hip's and motion_ops.hip's launchers behind dspfft_execute_spectrogram_* / _ispectrogram_*.  Weak, as above.
extern "C" __attribute__((weak, visibility("hidden"))) int dspfft_block_spec_launch(const dspfft::BlockSpecArgs *a, int inverse, int nwg, size_t lds, void *stream);
extern "C" __attribute__((weak, visibility("hidden"))) int dspfft_spec_blocks_launch(int inverse, int u8, void *d_pix, void *d_coeffs, const int n[3], const int minbuf_hw[2], size_t nblocks,
                                                                                      long long block_stride, const dspfft_motion_spec_params *sp, const dspfft_motion_filter_params *filter,
                                                                                      unsigned long long *d_coeffs_coded, void *stream);
// block_spec_packed.hip's and motion_spec_packed.hip's launchers behind dspfft_execute_spectrogram_u8_packed / _ispectrogram_u8_packed.  Weak, as above.
extern "C" __attribute__((weak, visibility("hidden"))) int dspfft_block_spec_packed_launch(const dspfft::BlockSpecPackedArgs *a, int inverse, int nwg, size_t lds, void *stream);
extern "C" __attribute__((weak)) int dspfft_motion_filter_packed(float *d_coeffs, int h, int w, int components, size_t frames, const dspfft_motion_filter_params *filter,
                                                                 const dspfft_motion_packed *packed, unsigned long long *d_coeffs_coded, void *stream);   // motion_filter_packed.hip
extern "C" __attribute__((weak, visibility("hidden"))) int dspfft_spec_frames_packed_launch(int inverse, uint8_t *d_pix, float *d_coeffs, int h, int w, int components, size_t frames,
                                                                                       const dspfft_motion_spec_params *sp, const dspfft_motion_filter_params *filter,
                                                                                       const dspfft_motion_packed *packed, unsigned long long *d_coeffs_coded, void *stream);
extern "C" __attribute__((weak, visibility("hidden"))) int dspfft_row_u8_trc_launch(int row_spec_id, const dspfft::PassArgs *a, const dspfft::U8IOTrc *io, int nwg, void *stream);
// spec_image.hip's two sweeps and spec_inst_row_u8c.hip's interleaved 8-bit row ends behind dspfft_execute_spec_u8 / _ispec_u8.  Weak, as above.
extern "C" __attribute__((weak, visibility("hidden"))) int dspfft_spec_image_encode_launch(const dspfft::SpecImageEnc *a, void *stream);
extern "C" __attribute__((weak, visibility("hidden"))) int dspfft_spec_image_decode_launch(const dspfft::SpecImageDec *a, void *stream);
extern "C" __attribute__((weak, visibility("hidden"))) int dspfft_row_u8c_has(int row_spec_id);
extern "C" __attribute__((weak, visibility("hidden"))) int dspfft_row_u8c_launch(int row_spec_id, const dspfft::PassArgs *a, const dspfft::U8IO *io, int nwg, void *stream);

static thread_local char g_err[512] = "";
static int fail(int code, const char *fmt, ...)
{
	va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap);
	return code;
}
extern "C" const char *dspfft_last_error(void) { return g_err; }
extern "C" const char *dspfft_version(void) { return "dspfft 0.1 (gfx950)"; }

namespace {

struct Dim { int n; long long is, os; };

const int kRadices[] = {16, 15, 13, 12, 11, 10, 9, 8, 7, 6, 5, 4, 3, 2};

// Smallest number of stages, then smallest sum of radices (less butterfly work / registers).
bool factor_search(int L, int depth, int maxdepth, std::vector<int> &cur, std::vector<int> &best, int &bestsum, int minr)
{
	if (L == 1) {
		int s = 0; for (int r : cur) s += r;
		if (best.empty() || cur.size() < best.size() || (cur.size() == best.size() && s < bestsum)) { best = cur; bestsum = s; }
		return true;
	}
	if (depth == maxdepth) return false;
	bool ok = false;
	for (int r : kRadices) {
		if (r > minr) continue;          // non-increasing order: each multiset visited once
		if (L % r) continue;
		cur.push_back(r);
		ok |= factor_search(L / r, depth + 1, maxdepth, cur, best, bestsum, r);
		cur.pop_back();
	}
	return ok;
}

bool factorize(int L, std::vector<int> &radices)
{
	radices.clear();
	if (L == 1) return true;
	for (int maxdepth = 1; maxdepth <= 8; maxdepth++) {
		std::vector<int> cur, best; int bestsum = 0;
		if (factor_search(L, 0, maxdepth, cur, best, bestsum, 16)) {
			// largest radix last: the last stage needs no twiddles
			std::sort(best.begin(), best.end());
			radices = best;
			return true;
		}
	}
	return false;
}

FastDiv make_div(uint32_t d)
{
	FastDiv f; f.d = d; f.mul = d >= 2 ? (uint32_t)((((uint64_t)1 << 32) + d - 1) / d) : 0; return f;
}

// Tuning overrides for experiments and A/B runs (0 / unset = the built-in choice).  plan_finish() takes a snapshot of the planner switches listed
// here (EnvScope) and everything it calls -- build_pass, build_split, build_block -- consults only that, so the passes of a plan are made under one
// consistent set of values whatever other threads do meanwhile.  The slice plans that a roundtrip over a clip makes later
// (slice_plan) are made under their parent's snapshot and planning effort, which the plan keeps.  What acts OUTSIDE plan_finish reads the environment
// where it acts.  On every call: DSPFFT_NO_FUSED_ROUNDTRIP (fused_roundtrip_off), DSPFFT_ROW_CHAN and dspfft_plan_scan_prepare's DSPFFT_SCAN_EIDS
// and DSPFFT_ZSKIP.  Once per process, at the first use: DSPFFT_LEAN01, DSPFFT_RT_SLICE and DSPFFT_RT_STREAMS (slice_switches).
const char *const kPlanEnv[] = {"DSPFFT_JIT", "DSPFFT_JIT_TUNE", "DSPFFT_NO_TINY", "DSPFFT_ROW_LPW", "DSPFFT_ROW_THREADS", "DSPFFT_COL_K", "DSPFFT_COL_THREADS",
                                "DSPFFT_DENSE_STAGED", "DSPFFT_NO_SPLIT", "DSPFFT_FORCE_SPLIT", "DSPFFT_NO_BLOCK", "DSPFFT_BLOCK_G", "DSPFFT_NO_BLUESTEIN"};
constexpr int kNPlanEnv = (int)(sizeof kPlanEnv / sizeof kPlanEnv[0]);
thread_local const int *t_plan_env = nullptr;
struct EnvScope {
	int v[kNPlanEnv];
	const int *prev;
	// the environment as it is now, or `stored` (a plan's plan_env); an enclosing scope's values hold in a scope opened inside it
	explicit EnvScope(const int *stored = nullptr) : prev(t_plan_env)
	{
		if (!stored) stored = prev;
		for (int i = 0; i < kNPlanEnv; i++) { const char *e = stored ? nullptr : getenv(kPlanEnv[i]); v[i] = stored ? stored[i] : e ? atoi(e) : 0; }
		t_plan_env = v;
	}
	~EnvScope() { t_plan_env = prev; }
};
int env_int(const char *name)
{
	if (t_plan_env) for (int i = 0; i < kNPlanEnv; i++) if (!strcmp(name, kPlanEnv[i])) return t_plan_env[i];
	const char *e = getenv(name);
	return e ? atoi(e) : 0;
}

struct Tables {
	void *T = nullptr, *W = nullptr, *pos = nullptr, *cosTab = nullptr;
	void *WM = nullptr, *chirp = nullptr, *Bhat = nullptr;     // Bluestein (BLUE passes)
	void *H = nullptr;                                         // half-tile column passes: exp(-2 pi i n / N), n < N/2
	void *stage = nullptr;                                     // DENSE passes on lines longer than LDS holds: [line][N] staging copy
	void release()
	{
		be_free(T); be_free(W); be_free(pos); be_free(cosTab); be_free(WM); be_free(chirp); be_free(Bhat); be_free(H); be_free(stage);
		T = W = pos = cosTab = WM = chirp = Bhat = H = stage = nullptr;
	}
};

bool build_fft(int L, FftDesc &F, std::vector<uint32_t> &pos)
{
	std::vector<int> rad;
	if (!factorize(L, rad)) return false;
	F.L = L; F.ns = (int)rad.size();
	int Lc = L;
	for (int i = 0; i < F.ns; i++) {
		StageDesc &S = F.st[i];
		S.R = rad[i]; S.Lc = Lc; S.M1 = Lc / rad[i]; S.twstep = L / Lc; S.divM1 = make_div((uint32_t)S.M1);
		Lc = S.M1;
	}
	// digit reversal: slot p = sum d_i * (L / (R_1..R_i)) holds output k = d_1 + R_1 (d_2 + R_2 (...))
	pos.assign(L, 0);
	for (int p = 0; p < L; p++) {
		int rem = p, k = 0, mult = 1, span = L;
		for (int i = 0; i < F.ns; i++) {
			span /= rad[i];
			int d = rem / span; rem -= d * span;
			k += d * mult; mult *= rad[i];
		}
		pos[k] = (uint32_t)p;
	}
	return true;
}

struct Pass {
	enum Type { ROW, COL, DENSE, BLUE, TINY } type;   // BLUE = COL geometry, tile DFT by Bluestein's convolution; TINY = one line per thread
	TinyGeom tg;
	int blueM = 0;
	FftDesc fftM;
	int axis;
	bool first;
	PassGeom pa;               // typed pointers, tables and scales are filled in per launch (run_pass)
	DenseGeom da;
	LaunchGeom g;
	bool has_spec = false;     // a compile-time-specialised kernel also covers this pass ...
	PassGeom spa;              // ... with this geometry (used when the buffers are 16-B aligned)
	SpecInfo spec;
	int spec_nwg = 0;
	// outer-radix-2 split of a long column axis (dct_spec.h ColHalfSpec): the row pass works on row pairs, the column pass on half tiles
	bool pair = false, half = false;
	int pair_id = -1;
	SpecInfo hspec;
	PassGeom hpa;
	int half_nwg = 0;
	// a kernel compiled at plan time for this pass's geometry (jit_kernels.h; DSPFFT_JIT=1) where spec_list.h has no entry: spa /
	// spec_nwg describe it like a listed one's, jit_fn is this pass's kind
	bool jit = false;
	void *jit_fn = nullptr;
	void *jit_fn_u8 = nullptr;      // planar rows: the 8-bit variant of this pass's kind
	void *jit_fn_rt = nullptr;      // columns: the fused forward -> filter -> inverse kernel
	std::string jit_type;
	int jit_nthr = 0;
	std::vector<Dim> hostloop;
	Tables tab;
	std::string desc;
};

}  // namespace

struct dspfft_plan_s {
	int rank, howmany;
	int n[3], kinds[3];
	Dim axes[3];
	std::vector<Dim> batches;  // howmany/dist (one entry) or the guru interface's howmany_dims
	bool f64;                  // samples are double (dspfft_plan_many_r2r_f64): double tables; specialised kernels for the sizes of DSPFFT_*_SPECS_F64
	double scale, in0[3], out0[3];
	std::vector<Pass> passes;
	std::vector<Pass> split;   // alternative pass list of dspfft_execute / dspfft_execute_pass (build_split); empty when not applicable
	int split_col_axis = -1;
	// small blocks: all axes in one pass (block_core.h, build_block); used by dspfft_execute on 16-byte aligned buffers
	bool has_block = false;
	BlockGeom blk;
	int blk_kind = 0;
	int blk_axis[3];           // plan axis behind the block's x, y, z
	int blk_nwg = 0;
	size_t blk_lds = 0;
	std::string blk_desc;
	size_t alg_bytes;
	// sparse scan frames (PassGeom::zflags): per-tile flags of the masked column pass + a page of zeros, allocated on first use
	void *zflags = nullptr;
	size_t zflags_bytes = 0;
	void *zpage = nullptr;
	// dspfft_plan_scan_prepare: (min, max) owner id per column tile for the owner-id array `zr_ids` (elements per id zr_div), laid out
	// for the split passes (zr_split) or the plain ones
	void *zranges = nullptr;
	size_t zranges_bytes = 0;
	const void *zr_ids = nullptr;
	int zr_div = 0;
	bool zr_split = false;
	// ... and, for single-precision plans, the owner id of every element in the column tiles' reading order (PassGeom::eids), eid_bytes each
	void *eids = nullptr;
	size_t eids_bytes = 0;
	int eid_bytes = 0;         // 0: not built (the column pass reads zr_ids itself)
	// dspfft_plan_set_input_window: rows of `win_axis` outside [win_lo, win_hi) are zero by contract (first pass, specialised COL REDFT01)
	int win_axis = -1, win_lo = 0, win_hi = 0;
	int alt_axis = -1;         // dspfft_plan_set_output_alternate
	int mod_axis = -1, mod_rev = 0;          // dspfft_plan_set_input_modulation
	const void *mod_table = nullptr;
	bool first_axis_first = false;           // pass order (dspfft_plan_many_r2r_ordered): what a slice plan of this plan is built with
	int col_kpref = 0;                       // column tile width asked of be_find_spec first (slice plans: the narrow tile, see RtSlices)
	// dspfft_plan_set_u8_trc: the transfer characteristic of this plan's 8-bit end and its tables on the device (a TrcU8Tab; a slice plan
	// borrows its parent's)
	int u8_trc = 0;
	void *u8_tab = nullptr;
	bool u8_tab_owned = false;
	// dspfft_execute_roundtrip_u8 over a clip of frames: plans for a slice of the clip whose float intermediate the Infinity Cache holds
	// (roundtrip_core), built on first use and owned by the forward plan
	struct RtSlices {
		const dspfft_plan_s *inv_of = nullptr; int frames = 0;
		dspfft_plan_s *fwd = nullptr, *inv = nullptr, *fwd_rem = nullptr, *inv_rem = nullptr;
		void *side = nullptr, *ev_fork = nullptr, *ev_join = nullptr;
		RtSlices() = default;
		RtSlices(const RtSlices &) = delete;
		RtSlices &operator=(const RtSlices &) = delete;
		~RtSlices()
		{
			for (dspfft_plan_s *q : {fwd, inv, fwd_rem, inv_rem}) dspfft_destroy_plan(q);
			if (side) be_stream_destroy(side);
			for (void *e : {ev_fork, ev_join}) if (e) be_event_destroy(e);
		}
	};
	std::vector<std::unique_ptr<RtSlices>> rt_slices;
	// a roundtrip over blocks along time (rt_temporal): this plan's axis as a complex FFT of its full length with the column pass's tables
	// (the plan's own pass has none when it is a TINY or DENSE pass), built on first use under rt_mutex
	std::unique_ptr<Pass> temporal;
	std::mutex rt_mutex;                     // two host threads may run the same plan pair on their own buffers and streams: the slice plans are made once, and
	                                         // a call's fork / slices / join are enqueued as one piece (the library stream and its two events are shared)
	// what plan_finish made this plan under: the planning effort and the planner's switches (EnvScope); its slice plans are made under the same
	int plan_effort = 0;
	int plan_env[kNPlanEnv];
};

namespace {

void merge_dims(std::vector<Dim> &d)
{
	std::sort(d.begin(), d.end(), [](const Dim &a, const Dim &b) { return a.os < b.os; });
	for (size_t i = 0; i + 1 < d.size();) {
		if (d[i + 1].is == d[i].n * d[i].is && d[i + 1].os == d[i].n * d[i].os) {
			d[i].n *= d[i + 1].n; d.erase(d.begin() + i + 1);
		} else i++;
	}
}

// T and W in the plan's sample type (computed in long double either way); the pass keeps them as void* in
// P.tab and run_pass hands them to the kernel arguments of the matching type
template <class R>
int upload_tables_t(Pass &P, int N, int L, const std::vector<uint32_t> &pos)
{
	const long double pi = 3.14159265358979323846264338327950288L;
	std::vector<cx<R>> T(N + 1), W(std::max(L, 1));
	for (int j = 0; j <= N; j++) T[j] = cmk<R>((R)cosl(pi * j / (2.0L * N)), (R)-sinl(pi * j / (2.0L * N)));
	for (int t = 0; t < L; t++) W[t] = cmk<R>((R)cosl(2 * pi * t / L), (R)-sinl(2 * pi * t / L));
	P.tab.T = be_alloc(T.size() * sizeof(cx<R>));
	P.tab.W = be_alloc(W.size() * sizeof(cx<R>));
	P.tab.pos = be_alloc(pos.size() * sizeof(uint32_t));
	if (!P.tab.T || !P.tab.W || !P.tab.pos) return -1;
	if (be_upload(P.tab.T, T.data(), T.size() * sizeof(cx<R>))) return -1;
	if (be_upload(P.tab.W, W.data(), W.size() * sizeof(cx<R>))) return -1;
	if (be_upload(P.tab.pos, pos.data(), pos.size() * sizeof(uint32_t))) return -1;
	P.pa.pos = (const uint32_t *)P.tab.pos;
	return 0;
}
int upload_tables(Pass &P, bool f64, int N, int L, const std::vector<uint32_t> &pos)
{
	return f64 ? upload_tables_t<double>(P, N, L, pos) : upload_tables_t<float>(P, N, L, pos);
}

// ---- Bluestein tables --------------------------------------------------------------------------
typedef std::complex<long double> cld;
const long double kPiL = 3.14159265358979323846264338327950288L;

// in-place forward DFT of any length whose prime factors are small (recursive decimation in time; host, plan time)
void host_fft(std::vector<cld> &x)
{
	const size_t n = x.size();
	if (n <= 1) return;
	size_t r = n;
	for (size_t f = 2; f * f <= n; f++) if (n % f == 0) { r = f; break; }
	const size_t m = n / r;
	std::vector<std::vector<cld>> sub(r, std::vector<cld>(m));
	for (size_t j = 0; j < r; j++) for (size_t i = 0; i < m; i++) sub[j][i] = x[i * r + j];
	for (size_t j = 0; j < r; j++) host_fft(sub[j]);
	std::vector<cld> w(n);
	for (size_t t = 0; t < n; t++) w[t] = cld(cosl(2 * kPiL * t / n), -sinl(2 * kPiL * t / n));
	for (size_t k = 0; k < n; k++) {
		cld acc = 0;
		for (size_t j = 0; j < r; j++) acc += w[(j * k) % n] * sub[j][k % m];
		x[k] = acc;
	}
}

// convolution length: 7-smooth M in [lo, 1.3 lo] minimising (stages x M) -- every stage is one pass over the M-row
// LDS buffer -- e.g. lo = 2731: 2880 = 12x15x16 (3 stages) beats 2744 = 7x7x7x8 (4 stages of costlier butterflies).
// DSPFFT_NO_BLUESTEIN=1 (plan time) disables the path (the O(N^2) DENSE kernel takes over; used by its tests).
int blue_length(int lo, FftDesc &F, std::vector<uint32_t> &pos)
{
	if (env_int("DSPFFT_NO_BLUESTEIN") == 1) return 0;
	int best = 0; long long bestcost = 0;
	for (int M = lo; M <= lo + lo / 3 + 16; M++) {
		int r = M;
		for (int p : {2, 3, 5, 7}) while (r % p == 0) r /= p;
		if (r != 1) continue;
		FftDesc f; std::vector<uint32_t> q;
		if (!build_fft(M, f, q)) continue;
		const long long cost = (long long)f.ns * M;
		if (!best || cost < bestcost) { best = M; bestcost = cost; }
	}
	if (best) build_fft(best, F, pos);
	return best;
}

template <class R>
int upload_blue_tables_t(Pass &P, int N, int M, const std::vector<uint32_t> &posM)
{
	std::vector<cld> c(N), b(M, cld(0));
	for (long long n = 0; n < N; n++) {
		const long long r = (n * n) % (2LL * N);                    // exact phase reduction
		c[n] = cld(cosl(kPiL * r / N), sinl(kPiL * r / N));
	}
	b[0] = c[0];
	for (int m = 1; m < N; m++) { b[m] = c[m]; b[M - m] = c[m]; }
	host_fft(b);
	std::vector<cx<R>> T(N + 1), WM(M), chirp(N), Bhat(M);
	std::vector<uint32_t> ident(N);
	for (int j = 0; j <= N; j++) T[j] = cmk<R>((R)cosl(kPiL * j / (2.0L * N)), (R)-sinl(kPiL * j / (2.0L * N)));
	for (int t = 0; t < M; t++) WM[t] = cmk<R>((R)cosl(2 * kPiL * t / M), (R)-sinl(2 * kPiL * t / M));
	for (int n = 0; n < N; n++) { chirp[n] = cmk<R>((R)c[n].real(), (R)c[n].imag()); ident[n] = (uint32_t)n; }
	for (int k = 0; k < M; k++) Bhat[posM[k]] = cmk<R>((R)(b[k].real() / M), (R)(b[k].imag() / M));   // digit-reversed, like the spectrum it multiplies
	struct { void **dst; const void *src; size_t bytes; } up[] = {
		{&P.tab.T, T.data(), T.size() * sizeof(cx<R>)}, {&P.tab.WM, WM.data(), WM.size() * sizeof(cx<R>)},
		{&P.tab.chirp, chirp.data(), chirp.size() * sizeof(cx<R>)}, {&P.tab.Bhat, Bhat.data(), Bhat.size() * sizeof(cx<R>)},
		{&P.tab.pos, ident.data(), ident.size() * sizeof(uint32_t)}};
	for (auto &u : up) {
		*u.dst = be_alloc(u.bytes);
		if (!*u.dst || be_upload(*u.dst, u.src, u.bytes)) return -1;
	}
	P.pa.pos = (const uint32_t *)P.tab.pos;
	return 0;
}

std::string radix_string(const FftDesc &F)
{
	std::string s;
	for (int i = 0; i < F.ns; i++) { if (i) s += "x"; s += std::to_string(F.st[i].R); }
	return s.empty() ? "1" : s;
}

// Build the pass along transformed axis `a`.  `first` => reads the user's input strides.
// ---- plan-time specialisation (DSPFFT_JIT=1) ----
// Radix order and thread count for a length without an entry in spec_list.h, by the rules the listed entries came out of
// (tools/kbench*, colbench, wavebench): largest radix first, an odd radix last when there is one (conflict-free last stage);
// about 11 samples (ROW, at most 512 threads while two lines fit a CU) / 34 samples (COL) of the tile per thread, rounded to a power of two.
std::string jit_radices(const FftDesc &F)
{
	std::vector<int> r;
	for (int i = 0; i < F.ns; i++) r.push_back(F.st[i].R);
	std::sort(r.begin(), r.end(), [](int x, int y) { return x > y; });
	int odd = -1;
	for (int i = (int)r.size() - 1; i >= 0; i--) if (r[i] % 2) { odd = i; break; }
	if (odd >= 0) { const int v = r[odd]; r.erase(r.begin() + odd); r.push_back(v); }
	std::string s;
	for (int v : r) s += ", " + std::to_string(v);
	return s;
}
int jit_threads(double want)
{
	int t = 64;
	while (t < 1024 && (double)t * 1.41 < want) t *= 2;
	return t;
}
std::string library_dir()
{
	Dl_info info;
	if (!dladdr((const void *)&library_dir, &info) || !info.dli_fname) return ".";
	std::string p = info.dli_fname;
	const size_t k = p.rfind('/');
	return k == std::string::npos ? "." : p.substr(0, k);
}
// DSPFFT_JIT=1 forces it on, =2 off; otherwise the planning effort the caller asked for decides (dspfft_set_plan_effort: the FFTW
// shim passes FFTW_MEASURE / PATIENT / EXHAUSTIVE on as "this plan will be executed many times", FFTW_ESTIMATE as "plan fast")
// planning effort of the plans made next: a PROCESS-WIDE value (dspfft_set_plan_effort: what one thread sets, plans made on any thread see -- worker
// pools, Python threads) that a thread may override for itself (dspfft_set_thread_plan_effort; < 0: no override).  The FFTW shim's set / plan /
// restore around one fftw(plan_many_r2r) call (fftw_shim.hip make_plan) uses the thread's override, so it cannot leak into a plan another thread
// is making.  (Round 5 made the one setter thread-local, which silently dropped plans created on other threads to effort 0: ADVICE r05.)
std::atomic<int> g_plan_effort_default{0};
thread_local int t_plan_effort = -1;
#define g_plan_effort (t_plan_effort >= 0 ? t_plan_effort : g_plan_effort_default.load(std::memory_order_relaxed))
bool jit_enabled()
{
	const int e = env_int("DSPFFT_JIT");
	return be_jit_available() && (e == 1 || (e != 2 && g_plan_effort > 0));
}

// Planning effort 2 (FFTW_PATIENT / FFTW_EXHAUSTIVE, DSPFFT_JIT_TUNE=1): compile a handful of candidates -- the rule's choice, the
// planner's own radix order, half and twice the threads, the next narrower column tile -- run each on a scratch buffer laid out like
// the plan's data and keep the fastest.  Every candidate lands in the disk cache; only the timing (milliseconds) is repeated later.
struct JitCand { std::string type; int T, K; };
bool jit_tune() { return env_int("DSPFFT_JIT_TUNE") == 1 || (env_int("DSPFFT_JIT_TUNE") != 2 && g_plan_effort >= 2); }
std::string planner_radices(const FftDesc &F)
{
	std::string s;
	for (int i = 0; i < F.ns; i++) s += ", " + std::to_string(F.st[i].R);
	return s;
}
size_t plan_span(const dspfft_plan_s *pl)
{
	long long span = 1;
	for (int a = 0; a < pl->rank; a++) span += (long long)(pl->n[a] - 1) * std::max(pl->axes[a].is, pl->axes[a].os);
	for (const Dim &b : pl->batches) span += (long long)(b.n - 1) * std::max(b.is, b.os);
	return (size_t)span;
}
template <class R> void fill_args(PassArgsT<R> &a, const PassGeom &g, const dspfft_plan_s *pl, const Pass &P, const R *in, R *out, double scale, const struct Fuse &fz);
template <class R>
float jit_time_t(const dspfft_plan_s *pl, const Pass &P, const PassGeom &g, void *fn, int nwg, int nthr, void *scratch);

// fills P.jit* with the (fastest) candidate that compiles; geometry of candidate i through `geom(i, g, nwg)`
template <class G>
bool jit_pick(const dspfft_plan_s *pl, Pass &P, int is_col, const std::vector<JitCand> &cands, int kind, G geom, JitCand &chosen)
{
	const std::string dir = library_dir();
	const bool tune = jit_tune() && cands.size() > 1;
	void *scratch = nullptr;
	if (tune) {
		const size_t bytes = plan_span(pl) * (pl->f64 ? 8 : 4);
		scratch = be_alloc(bytes);
		if (scratch && be_zero(scratch, bytes, nullptr)) { be_free(scratch); scratch = nullptr; }
	}
	float best = 0.f;
	bool have = false;
	// single precision: columns also get the fused roundtrip, planar rows of a multiple of four samples the 8-bit variants
	const int extras = !pl->f64 && (is_col || (P.pa.C == 1 && P.pa.N % 4 == 0));
	for (size_t i = 0; i < cands.size(); i++) {
		void *fn[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
		char log[2048] = "";
		const int nfn = be_jit_build(cands[i].type.c_str(), is_col, extras, dir.c_str(), fn, log, sizeof log);
		if (nfn < 2) {
			if (i == 0) fprintf(stderr, "dspfft: plan-time compilation of %s failed\n%s\n", cands[i].type.c_str(), log);
			continue;
		}
		PassGeom g = P.pa;
		int nwg = 0;
		geom(cands[i], g, nwg);
		float ms = 0.f;
		if (tune && scratch) {
			ms = pl->f64 ? jit_time_t<double>(pl, P, g, fn[kind], nwg, cands[i].T, scratch) : jit_time_t<float>(pl, P, g, fn[kind], nwg, cands[i].T, scratch);
			if (ms <= 0.f) continue;
		}
		if (!have || (tune && scratch && ms < best)) {
			have = true; best = ms; chosen = cands[i];
			P.jit = true; P.jit_fn = fn[kind]; P.jit_nthr = cands[i].T; P.spa = g; P.spec_nwg = nwg; P.jit_type = cands[i].type;
			P.jit_fn_u8 = (!is_col && nfn == 4) ? fn[2 + kind] : nullptr;
			P.jit_fn_rt = (is_col && nfn == 3) ? fn[2] : nullptr;
		}
		if (!(tune && scratch)) break;
	}
	be_free(scratch);
	return have;
}

// ROW: exact (N, C).  Returns true and fills P.jit* on success.
bool jit_row(const dspfft_plan_s *pl, Pass &P, int N, int C, long long nlines, const FftDesc &F, int kind)
{
	const size_t es = pl->f64 ? 8 : 4;
	const size_t lds = (size_t)C * (N / 2 + 16) * 2 * es;
	if (F.ns < 1 || lds > be_max_lds()) return false;
	// (the timed search of planning effort 2 kept picking twice the threads of the first rule, N C / 22, for RGB rows of 1500-2400
	// pixels and never more than 512 below 4000 pixels)
	int T0 = jit_threads((double)N * C / 11.0);
	if (T0 > 512 && lds <= 80 * 1024) T0 = 512;
	const std::string head = std::string("RowSpecT<") + (pl->f64 ? "double" : "float") + ", " + std::to_string(N) + ", " + std::to_string(C) + ", ";
	std::vector<JitCand> cands;
	auto add = [&](int T, const std::string &rad) {
		if (T < 64 || T > 1024) return;
		JitCand c{head + std::to_string(T) + rad + ">", T, 0};
		for (const JitCand &o : cands) if (o.type == c.type) return;
		cands.push_back(c);
	};
	add(T0, jit_radices(F)); add(T0, planner_radices(F)); add(T0 * 2, jit_radices(F)); add(T0 / 2, jit_radices(F)); add(T0 * 2, planner_radices(F));
	JitCand c;
	if (!jit_pick(pl, P, 0, cands, kind, [&](const JitCand &, PassGeom &, int &nwg) { nwg = (int)nlines; }, c)) return false;
	char buf[320];
	snprintf(buf, sizeof buf, "axis %d: ROW+%s N=%d C=%d compiled at plan time: %s, lines=%lld", P.axis, pl->f64 ? " f64" : "", N, C, c.type.c_str(), nlines);
	P.desc = buf;
	return true;
}
// COL: tile width by the LDS it takes (16 samples up to 80 KB, then 8, then 4; doubles half of that), the inner extent a multiple of it
bool jit_col(const dspfft_plan_s *pl, Pass &P, int N, int inner, const FftDesc &F, int kind)
{
	const size_t es = pl->f64 ? 8 : 4;
	const int Kmax = pl->f64 ? 8 : 16, Kmin = pl->f64 ? 2 : 4;
	int K = Kmax;
	while (K >= Kmin && ((size_t)(N + 16) * K * es > (K == Kmax ? 80u * 1024 : 150u * 1024) || inner % K)) K /= 2;
	if (K < Kmin || F.ns < 1) return false;
	const std::string head = std::string("ColSpecT<") + (pl->f64 ? "double" : "float") + ", " + std::to_string(N) + ", ";
	std::vector<JitCand> cands;
	auto add = [&](int k, int T, const std::string &rad) {
		if (k < Kmin || inner % k || T < 64 || T > 1024 || (size_t)(N + 16) * k * es > 150u * 1024) return;
		JitCand c{head + std::to_string(k) + ", " + std::to_string(T) + rad + ">", T, k};
		for (const JitCand &o : cands) if (o.type == c.type) return;
		cands.push_back(c);
	};
	auto threads = [&](int k) { return jit_threads((double)N * k * (pl->f64 ? 2 : 1) / 34.0); };
	add(K, threads(K), jit_radices(F)); add(K, threads(K), planner_radices(F)); add(K, threads(K) * 2, jit_radices(F)); add(K, threads(K) / 2, jit_radices(F));
	add(K / 2, threads(K / 2), jit_radices(F)); add(K * 2, threads(K * 2), jit_radices(F));
	JitCand c;
	if (!jit_pick(pl, P, 1, cands, kind, [&](const JitCand &cd, PassGeom &g, int &nwg) { g.K = cd.K; g.B = cd.K / 2; g.ntiles = inner / cd.K; nwg = g.ntiles * g.nb0 * g.nb1; }, c)) return false;
	char buf[320];
	snprintf(buf, sizeof buf, "axis %d: COL+%s N=%d K=%d compiled at plan time: %s, tiles=%d wgs=%d", P.axis, pl->f64 ? " f64" : "", N, c.K, c.type.c_str(), P.spa.ntiles, P.spec_nwg);
	P.desc = buf;
	return true;
}

int build_pass(dspfft_plan_s *pl, int a, bool first, Pass &P)
{
	memset(&P.pa, 0, sizeof P.pa); memset(&P.da, 0, sizeof P.da); memset(&P.g, 0, sizeof P.g);
	P.axis = a; P.first = first;
	const int N = pl->n[a];
	const int kind = pl->kinds[a] == DSPFFT_REDFT10 ? KIND_REDFT10 : KIND_REDFT01;
	auto eff = [&](const Dim &d) { Dim e = d; if (!first) e.is = d.os; return e; };
	const Dim ax = eff(pl->axes[a]);
	std::vector<Dim> others;
	for (int b = 0; b < pl->rank; b++) if (b != a && pl->n[b] > 1) others.push_back(eff(pl->axes[b]));
	for (const Dim &b : pl->batches) if (b.n > 1) others.push_back(eff(b));
	const size_t maxlds = be_max_lds();
	const size_t es = pl->f64 ? 8 : 4;         // bytes per sample; a complex LDS slot is 2*es
	const char *tag = pl->f64 ? " f64" : "";
	char buf[256];

	// ---------------- TINY ----------------
	if (N <= 32 && !(env_int("DSPFFT_NO_TINY") == 1)) {
		std::vector<Dim> d = others;
		merge_dims(d);
		long long nlines = 1;
		for (const Dim &x : d) nlines *= x.n;
		if (d.size() <= 6 && nlines < (1ll << 31)) {
			TinyGeom &tg = P.tg;
			memset(&tg, 0, sizeof tg);
			tg.N = N; tg.kind = kind; tg.es_in = ax.is; tg.es_out = ax.os; tg.nd = (int)d.size(); tg.nlines = nlines;
			for (size_t i = 0; i < d.size(); i++) { tg.bn[i] = d[i].n; tg.bis[i] = d[i].is; tg.bos[i] = d[i].os; tg.bdiv[i] = make_div((uint32_t)d[i].n); }
			// contiguous lines packed back to back: element-contiguous global access through LDS chunks
			tg.packed = d.size() >= 1 && ax.is == 1 && ax.os == 1 && d[0].is == N && d[0].os == N;
			tg.chunk_div = make_div((uint32_t)(tg.packed ? (d[0].n + TINY_CHUNK - 1) / TINY_CHUNK : 1));
			P.type = Pass::TINY;
			P.g.nwg = (int)((nlines + 255) / 256); P.g.nthr = 256; P.g.lds_bytes = 0;
			snprintf(buf, sizeof buf, "axis %d: TINY%s N=%d lines=%lld dims=%d%s", a, tag, N, nlines, tg.nd, tg.packed ? " packed" : "");
			P.desc = buf;
			return 0;
		}
	}
	// ---------------- ROW ----------------
	{
		bool ok = (N % 2 == 0) && ax.is == ax.os && ax.is >= 1 && ax.is <= 4;
		int C = (int)ax.is, cdim = -1;
		if (ok && C > 1) {
			ok = false;
			for (size_t i = 0; i < others.size(); i++)
				if (others[i].is == 1 && others[i].os == 1 && others[i].n == C) { cdim = (int)i; ok = true; }
		}
		FftDesc F; std::vector<uint32_t> pos;
		if (ok) ok = build_fft(N / 2, F, pos);
		if (ok) {
			const int L = N / 2;
			// the line's C signals sit in LDS together; longer lines go to the column pass -- unless the line has listed channel-line kernels
			// (one channel per workgroup: 7680 x 3 doubles, spec_list.h)
			if ((size_t)L * C * 2 * es > maxlds) {
				SpecInfo si;
				ok = pl->f64 && C > 1 && be_find_spec_f64(0, N, C, &si) && si.chan;
			}
			if (ok) {
				std::vector<Dim> lines;
				for (size_t i = 0; i < others.size(); i++) if ((int)i != cdim) lines.push_back(others[i]);
				merge_dims(lines);
				PassGeom &pa = P.pa;
				pa.N = N; pa.kind = kind; pa.C = C; pa.fft = F;
				pa.nb0 = lines.size() > 0 ? lines[0].n : 1; pa.sb0_in = lines.size() > 0 ? lines[0].is : 0; pa.sb0_out = lines.size() > 0 ? lines[0].os : 0;
				pa.nb1 = lines.size() > 1 ? lines[1].n : 1; pa.sb1_in = lines.size() > 1 ? lines[1].is : 0; pa.sb1_out = lines.size() > 1 ? lines[1].os : 0;
				const long long nb2 = lines.size() > 2 ? lines[2].n : 1;
				pa.sb2_in = lines.size() > 2 ? lines[2].is : 0; pa.sb2_out = lines.size() > 2 ? lines[2].os : 0;
				for (size_t i = 3; i < lines.size(); i++) P.hostloop.push_back(lines[i]);
				P.type = Pass::ROW;
				const long long nlines = (long long)pa.nb0 * pa.nb1 * nb2;
				pa.nlines = nlines;
				if (nlines > 0x7fffffffLL) return fail(-2, "too many lines for one launch");
				// short lines: several per workgroup (about 2048 samples), as long as the launch keeps well over a workgroup per CU
				int LPW = 1;
				while (LPW < 16 && (long long)N * C * LPW < 2048 && nlines / (2 * LPW) >= 1024 && (size_t)L * C * 2 * LPW * 2 * es <= maxlds) LPW *= 2;
				if (env_int("DSPFFT_ROW_LPW")) LPW = std::min(16, std::max(1, env_int("DSPFFT_ROW_LPW")));
				pa.LPW = LPW; pa.divB = make_div((uint32_t)(C * LPW)); pa.divC = make_div((uint32_t)C);
				pa.divNC = make_div((uint32_t)(N * C)); pa.divKC = make_div((uint32_t)((L / 2 + 1) * C));
				P.g.nwg = (int)((nlines + LPW - 1) / LPW); P.g.lds_bytes = (size_t)L * C * LPW * 2 * es;
				// about 16 waves per CU: one big-LDS workgroup of 1024 threads, two of 512, otherwise 256 (measured, tools/sweep_generic.py)
				P.g.nthr = P.g.lds_bytes > 80 * 1024 ? 1024 : P.g.lds_bytes > 24 * 1024 ? 512 : 256;
				if (env_int("DSPFFT_ROW_THREADS")) P.g.nthr = env_int("DSPFFT_ROW_THREADS");
				if (upload_tables(P, pl->f64, N, L, pos)) return fail(-3, "table upload failed");
				snprintf(buf, sizeof buf, "axis %d: ROW%s  N=%d C=%d fft=%d(%s) lines=%lld x%d lds=%zu", a, tag, N, C, L, radix_string(F).c_str(), nlines, LPW, P.g.lds_bytes);
				P.desc = buf;
				// vector pixel access needs the line starts aligned to the pixel vector (C=2: 8 B, C=4: 16 B)
				const int al = (C == 2 || C == 4) ? C : 1;
				bool aligned = true;
				for (const Dim &d : lines) aligned = aligned && (d.is % al == 0) && (d.os % al == 0);
				if (aligned && (pl->f64 ? be_find_spec_f64(0, N, C, &P.spec) : be_find_spec(0, N, C, &P.spec))) {
					P.has_spec = true; P.spa = pa; P.spec_nwg = (int)nlines;
					if (P.spec.chan) snprintf(buf, sizeof buf, "axis %d: ROW*%s N=%d C=%d spec#%d as %d channel lines, threads=%d lines=%lld lds=%zu", a, tag, N, C, P.spec.id, P.spec.chan, P.spec.nthr, nlines, P.spec.lds);
					else snprintf(buf, sizeof buf, "axis %d: ROW*%s N=%d C=%d spec#%d threads=%d lines=%lld lds=%zu", a, tag, N, C, P.spec.id, P.spec.nthr, nlines, P.spec.lds);
					P.desc = buf;
				} else if (aligned && jit_enabled() && lines.size() <= 2) {
					jit_row(pl, P, N, C, nlines, F, kind);
				}
				return 0;
			}
		}
	}
	// ---------------- COL (and its Bluestein variant) ----------------
	{
		FftDesc F, FM; std::vector<uint32_t> pos, posM;
		const bool direct = build_fft(N, F, pos);
		const int M = direct ? 0 : blue_length(2 * N - 1, FM, posM);
		bool ok = direct || M > 0;
		int idim = -1;
		for (size_t i = 0; i < others.size(); i++) if (others[i].is == 1 && others[i].os == 1) idim = (int)i;
		if (ok) {
			// merge dims that continue the inner run contiguously (dense embeddings)
			std::vector<Dim> rest;
			// no unit-stride dimension beside the axis (planar lines): a one-sample-wide "inner" run, i.e. tiles of one
			// real signal whose partner column is empty
			Dim inner = idim >= 0 ? others[idim] : Dim{1, 1, 1};
			for (size_t i = 0; i < others.size(); i++) if ((int)i != idim) rest.push_back(others[i]);
			std::sort(rest.begin(), rest.end(), [](const Dim &x, const Dim &y) { return x.os < y.os; });
			for (size_t i = 0; idim >= 0 && i < rest.size();) {
				if (rest[i].is == inner.n && rest[i].os == inner.n && (long long)inner.n * rest[i].n < (1 << 30)) { inner.n *= rest[i].n; rest.erase(rest.begin() + i); i = 0; }
				else i++;
			}
			merge_dims(rest);
			const size_t rows = direct ? (size_t)N : (size_t)M;           // complex LDS rows per tile column pair
			// tile width: 16 floats (64 B row segments); short axes take wider tiles so a workgroup still owns a few
			// thousand samples (a 64-row tile of width 16 is 1024 samples for 256 threads)
			int Kwant = 16;
			long long nbatch = 1;
			for (const Dim &d : rest) nbatch *= d.n;
			// ... as long as the launch still has well over a workgroup per CU (a single small frame keeps its narrow tiles)
			while (Kwant < 64 && (long long)rows * Kwant < 4096 && ((inner.n + 2 * Kwant - 1) / (2 * Kwant)) * nbatch >= 1024) Kwant *= 2;
			int K = std::min(env_int("DSPFFT_COL_K") ? env_int("DSPFFT_COL_K") : Kwant, (inner.n + 1) & ~1);
			while (K >= 2 && rows * (K / 2) * 2 * es > maxlds) K -= 2;
			if (K >= 2) {
				PassGeom &pa = P.pa;
				pa.N = N; pa.kind = kind; pa.K = K; pa.B = K / 2; pa.ninner = inner.n; pa.ntiles = (inner.n + K - 1) / K;
				pa.es_in = ax.is; pa.es_out = ax.os; pa.fft = F; pa.divB = make_div((uint32_t)pa.B);
				pa.nb0 = rest.size() > 0 ? rest[0].n : 1; pa.sb0_in = rest.size() > 0 ? rest[0].is : 0; pa.sb0_out = rest.size() > 0 ? rest[0].os : 0;
				pa.nb1 = rest.size() > 1 ? rest[1].n : 1; pa.sb1_in = rest.size() > 1 ? rest[1].is : 0; pa.sb1_out = rest.size() > 1 ? rest[1].os : 0;
				for (size_t i = 2; i < rest.size(); i++) P.hostloop.push_back(rest[i]);
				long long nwg = (long long)pa.ntiles * pa.nb0 * pa.nb1;
				if (nwg > 0x7fffffff) return fail(-2, "too many tiles for one launch");
				P.g.nwg = (int)nwg;
				P.g.lds_bytes = rows * pa.B * 2 * es;
				const long long slots = (long long)rows * pa.B;
				P.g.nthr = (slots >= 12000 || P.g.lds_bytes > 80 * 1024) ? 1024 : slots >= 4096 ? 512 : 256;   // measured, tools/sweep_generic.py
				if (env_int("DSPFFT_COL_THREADS")) P.g.nthr = env_int("DSPFFT_COL_THREADS");
				if (!direct) {
					P.type = Pass::BLUE; P.blueM = M; P.fftM = FM;
					memset(&pa.fft, 0, sizeof pa.fft);
					if (pl->f64 ? upload_blue_tables_t<double>(P, N, M, posM) : upload_blue_tables_t<float>(P, N, M, posM)) return fail(-3, "table upload failed");
					snprintf(buf, sizeof buf, "axis %d: BLUE%s N=%d K=%d inner=%d tiles=%d conv=%d(%s) wgs=%d lds=%zu", a, tag, N, K, inner.n, pa.ntiles, M, radix_string(FM).c_str(), P.g.nwg, P.g.lds_bytes);
					P.desc = buf;
					return 0;
				}
				P.type = Pass::COL;
				if (upload_tables(P, pl->f64, N, N, pos)) return fail(-3, "table upload failed");
				snprintf(buf, sizeof buf, "axis %d: COL%s  N=%d K=%d inner=%d tiles=%d fft=%d(%s) wgs=%d lds=%zu", a, tag, N, K, inner.n, pa.ntiles, N, radix_string(F).c_str(), P.g.nwg, P.g.lds_bytes);
				P.desc = buf;
				// float4 tile rows: every stride that positions a tile must keep 16-B alignment
				bool aligned = (ax.is % 4 == 0) && (ax.os % 4 == 0);
				for (const Dim &d : rest) aligned = aligned && (d.is % 4 == 0) && (d.os % 4 == 0);
				if (aligned && (pl->f64 ? be_find_spec_f64(1, N, inner.n, &P.spec) : be_find_spec(1, N, inner.n, &P.spec, pl->col_kpref))) {
					P.has_spec = true; P.spa = pa;
					P.spa.K = P.spec.P; P.spa.B = P.spec.P / 2; P.spa.ntiles = inner.n / P.spec.P;
					P.spec_nwg = P.spa.ntiles * pa.nb0 * pa.nb1;
					snprintf(buf, sizeof buf, "axis %d: COL*%s N=%d K=%d spec#%d threads=%d inner=%d tiles=%d wgs=%d lds=%zu (generic fallback: K=%d)", a, tag, N, P.spec.P, P.spec.id, P.spec.nthr, inner.n, P.spa.ntiles, P.spec_nwg, P.spec.lds, K);
					P.desc = buf;
				} else if (aligned && jit_enabled() && rest.size() <= 2) {
					jit_col(pl, P, N, inner.n, F, kind);
				}
				return 0;
			}
		}
	}
	// ---------------- DENSE ----------------
	{
		// a line longer than LDS holds (beyond Bluestein's range too: a prime factor > 13 in a length of tens of thousands) is staged in a
		// device array of the plan instead: the reference never checks for a NULL plan (spec/spec.c:63-64), so every length gets one
		const bool staged = (size_t)N * es > maxlds || env_int("DSPFFT_DENSE_STAGED") == 1;
		merge_dims(others);
		DenseGeom &da = P.da;
		da.N = N; da.kind = kind; da.es_in = ax.is; da.es_out = ax.os;
		da.nb0 = others.size() > 0 ? others[0].n : 1; da.sb0_in = others.size() > 0 ? others[0].is : 0; da.sb0_out = others.size() > 0 ? others[0].os : 0;
		da.nb1 = others.size() > 1 ? others[1].n : 1; da.sb1_in = others.size() > 1 ? others[1].is : 0; da.sb1_out = others.size() > 1 ? others[1].os : 0;
		da.nb2 = others.size() > 2 ? others[2].n : 1; da.sb2_in = others.size() > 2 ? others[2].is : 0; da.sb2_out = others.size() > 2 ? others[2].os : 0;
		for (size_t i = 3; i < others.size(); i++) P.hostloop.push_back(others[i]);
		const long double pi = 3.14159265358979323846264338327950288L;
		P.tab.cosTab = be_alloc((size_t)4 * N * es);
		if (!P.tab.cosTab) return fail(-3, "table upload failed");
		int urc;
		if (pl->f64) {
			std::vector<double> ct((size_t)4 * N);
			for (int t = 0; t < 4 * N; t++) ct[t] = (double)cosl(pi * t / (2.0L * N));
			urc = be_upload(P.tab.cosTab, ct.data(), ct.size() * 8);
		} else {
			std::vector<float> ct((size_t)4 * N);
			for (int t = 0; t < 4 * N; t++) ct[t] = (float)cosl(pi * t / (2.0L * N));
			urc = be_upload(P.tab.cosTab, ct.data(), ct.size() * 4);
		}
		if (urc) return fail(-3, "table upload failed");
		P.type = Pass::DENSE;
		long long lines = (long long)da.nb0 * da.nb1 * da.nb2;
		if (lines > 0x7fffffff) return fail(-2, "too many lines for the dense path");
		P.g.nwg = (int)lines; P.g.nthr = 256; P.g.lds_bytes = staged ? 0 : (size_t)N * es;
		if (staged) {
			// one staging array serves every host-loop iteration (they run one after the other); executions of this plan on two streams
			// at once would share it: dspfft_execute_many[_repeat] refuses that (staged_plan_on_two_streams)
			P.tab.stage = be_alloc((size_t)lines * N * es);
			if (!P.tab.stage) return fail(-3, "axis %d: no memory for the staging copy of %lld lines of %d samples", a, lines, N);
		}
		snprintf(buf, sizeof buf, "axis %d: DENSE%s N=%d lines=%lld lds=%zu%s", a, tag, N, lines, P.g.lds_bytes, staged ? " (lines staged in device memory)" : "");
		P.desc = buf;
		return 0;
	}
}

struct Fuse { const void *eids = nullptr; int eid_bytes = 0; const uint32_t *mask = nullptr; uint32_t id = 0, span = 1; int div = 1; bool accumulate = false; uint8_t *zflags = nullptr; int zshift = 0, zhalf = 0; const void *zpage = nullptr; const uint32_t *zranges = nullptr; };
FastDiv make_div(uint32_t d);

template <class R>
void fill_args(PassArgsT<R> &a, const PassGeom &g, const dspfft_plan_s *pl, const Pass &P, const R *in, R *out, double scale, const Fuse &fz)
{
	static_cast<PassGeom &>(a) = g;
	a.in = in; a.out = out; a.T = (const cx<R> *)P.tab.T; a.W = (const cx<R> *)P.tab.W; a.H = (const cx<R> *)P.tab.H;
	a.scale = (R)scale; a.in_scale0 = (R)pl->in0[P.axis]; a.out_scale0 = (R)pl->out0[P.axis];
	a.mask = fz.mask; a.mask_id = fz.id; a.mask_span = fz.span; a.mask_div = make_div((uint32_t)fz.div); a.accumulate = fz.accumulate;
	a.zflags = fz.zflags; a.zshift = fz.zshift; a.zhalf = fz.zhalf; a.zpage = fz.zpage; a.zranges = fz.zranges;
	// masked column tiles take their owner ids from the plan's element-order table where one was prepared for this id array and the range
	// starts below its saturated value; the range's end is clamped to that value (every id of such a table lies below it but DC's)
	a.mask_mode = 0; a.eids = nullptr;
	const uint32_t ones = fz.eid_bytes == 1 ? 0xffu : 0xffffu;
	if (fz.mask && fz.zpage && fz.eids && fz.eid_bytes && fz.id < ones) {
		a.mask_mode = fz.eid_bytes; a.eids = fz.eids;
		a.mask_span = (uint32_t)std::min<uint64_t>((uint64_t)fz.id + fz.span, ones) - fz.id;
	}
	a.alt_out = (pl->alt_axis == P.axis && pl->alt_axis >= 0) ? 1 : 0;
	static const int lean_off = []() { const char *e = getenv("DSPFFT_LEAN01"); return e && *e == '0' ? 1 : 0; }();
	a.lean_off = lean_off;
	a.win_lo = a.win_hi = 0;
	if (pl->win_axis == P.axis && P.first && !fz.mask && pl->zpage) { a.win_lo = pl->win_lo; a.win_hi = pl->win_hi; a.zpage = pl->zpage; }
	a.in_mul = nullptr; a.in_rev = 0;
	if (pl->mod_axis == P.axis && P.first && !fz.mask && a.win_hi > 0) { a.in_mul = pl->mod_table; a.in_rev = pl->mod_rev; }
}

// one candidate of the planning-effort-2 search: mean of three launches on the scratch buffer, in milliseconds (<= 0: failed)
template <class R>
float jit_time_t(const dspfft_plan_s *pl, const Pass &P, const PassGeom &g, void *fn, int nwg, int nthr, void *scratch)
{
	PassArgsT<R> a;
	fill_args(a, g, pl, P, (const R *)scratch, (R *)scratch, 1.0, Fuse());
	void *e0 = be_event_create(), *e1 = be_event_create();
	float ms = -1.f;
	if (e0 && e1 && !be_jit_launch(fn, &a, nwg, nthr, nullptr) && !be_event_record(e0, nullptr)) {
		bool ok = true;
		for (int i = 0; i < 3 && ok; i++) ok = !be_jit_launch(fn, &a, nwg, nthr, nullptr);
		if (ok && !be_event_record(e1, nullptr) && !be_event_synchronize(e1) && !be_event_elapsed_ms(e0, e1, &ms)) ms /= 3.f; else ms = -1.f;
	}
	be_event_destroy(e0); be_event_destroy(e1);
	return ms;
}
template float jit_time_t<float>(const dspfft_plan_s *, const Pass &, const PassGeom &, void *, int, int, void *);
template float jit_time_t<double>(const dspfft_plan_s *, const Pass &, const PassGeom &, void *, int, int, void *);

template <class R>
int run_pass(const dspfft_plan_s *pl, const Pass &P, const R *in, R *out, bool last, void *stream, const Fuse &fz = Fuse())
{
	const double scale = last ? pl->scale : 1.0;
	// iterate the host-side batch dims (rare: more batch levels than a kernel takes)
	std::vector<int> idx(P.hostloop.size(), 0);
	for (;;) {
		long long oin = 0, oout = 0;
		for (size_t i = 0; i < idx.size(); i++) { oin += idx[i] * P.hostloop[i].is; oout += idx[i] * P.hostloop[i].os; }
		int rc = 0;
		if (P.type == Pass::TINY) {
			TinyArgsT<R> a;
			static_cast<TinyGeom &>(a) = P.tg;
			a.in = in + oin; a.out = out + oout;
			a.scale = (R)scale; a.in_scale0 = (R)pl->in0[P.axis]; a.out_scale0 = (R)pl->out0[P.axis];
			a.mask = fz.mask; a.mask_id = fz.id; a.mask_span = fz.span; a.mask_div = make_div((uint32_t)fz.div); a.accumulate = fz.accumulate;
			rc = be_launch_tiny(a, stream);
		} else if (P.type == Pass::DENSE) {
			DenseArgsT<R> a;
			static_cast<DenseGeom &>(a) = P.da;
			a.in = in + oin; a.out = out + oout; a.cosTab = (const R *)P.tab.cosTab; a.stage = (R *)P.tab.stage;
			a.scale = (R)scale; a.in_scale0 = (R)pl->in0[P.axis]; a.out_scale0 = (R)pl->out0[P.axis];
			a.mask = fz.mask; a.mask_id = fz.id; a.mask_span = fz.span; a.mask_div = make_div((uint32_t)fz.div); a.accumulate = fz.accumulate;
			rc = be_launch_dense(a, P.g, stream);
		} else {
			bool use_spec = false;
			if constexpr (std::is_same<R, float>::value) {
				if (P.pair || P.half) {          // only reached through pick_passes(), which has checked alignment and scales
					PassArgs a;
					fill_args(a, P.pair ? P.spa : P.hpa, pl, P, in + oin, out + oout, scale, fz);
					rc = P.pair ? be_launch_row_pair(P.pair_id, a, P.spec_nwg / 2, stream) : be_launch_col_half(P.hspec.id, a, P.half_nwg, stream);
					if (rc) return fail(-4, "kernel launch failed (%s): backend code %d", P.desc.c_str(), rc);
					return 0;
				}
			}
			{
				// the specialised kernels move whole pixels (ROW: C samples) or four samples (COL) per access
				const uintptr_t al = sizeof(R) * (P.type == Pass::ROW ? (P.pa.C == 2 || P.pa.C == 4 ? P.pa.C : 1) : 4);
				const bool ptr_ok = ((al - 1) & ((uintptr_t)(in + oin) | (uintptr_t)(out + oout))) == 0;
				use_spec = (P.has_spec || P.jit) && ptr_ok;
				// the plan options that let a caller leave zeros unstored (input window), or that change values (modulation, alternating output
				// sign), live in the listed kernels only: a run that cannot take them must fail, not fall through to a kernel that ignores them
				const bool windowed = pl->win_axis == P.axis && P.first && pl->win_hi > 0;
				const bool alternating = pl->alt_axis >= 0 && pl->alt_axis == P.axis;
				if ((windowed || alternating) && !(P.has_spec && !P.jit && ptr_ok))
					return fail(-1, "%s: the plan's input window / modulation / alternating output need 16-byte aligned buffers (in %p, out %p): the listed kernel cannot run and no other honours them",
					            P.desc.c_str(), (const void *)(in + oin), (const void *)(out + oout));
				if (windowed && fz.mask)
					return fail(-1, "%s: an owner-id mask cannot be combined with an input window (the masked loads would read the rows the window leaves unstored)", P.desc.c_str());
				if (use_spec) {
					PassArgsT<R> a;
					fill_args(a, P.spa, pl, P, in + oin, out + oout, scale, fz);
					rc = P.jit ? be_jit_launch(P.jit_fn, &a, P.spec_nwg, P.jit_nthr, stream) : be_launch_spec(P.type == Pass::COL, P.spec.id, a, P.spec_nwg, stream);
				}
			}
			if (P.type == Pass::BLUE) {
				BlueArgsT<R> a;
				fill_args(a, P.pa, pl, P, in + oin, out + oout, scale, fz);
				a.M = P.blueM; a.fftM = P.fftM;
				a.WM = (const cx<R> *)P.tab.WM; a.chirp = (const cx<R> *)P.tab.chirp; a.Bhat = (const cx<R> *)P.tab.Bhat;
				rc = be_launch_blue(a, P.g, stream);
			} else if (!use_spec) {
				PassArgsT<R> a;
				fill_args(a, P.pa, pl, P, in + oin, out + oout, scale, fz);
				rc = P.type == Pass::ROW ? be_launch_row(a, P.g, stream) : be_launch_col(a, P.g, stream);
			}
		}
		if (rc) return fail(-4, "kernel launch failed (%s): backend code %d", P.desc.c_str(), rc);
		size_t i = 0;
		for (; i < idx.size(); i++) { if (++idx[i] < P.hostloop[i].n) break; idx[i] = 0; }
		if (i == idx.size()) break;
	}
	return 0;
}

}  // namespace

namespace {
// Outer radix-2 split of a long column axis for 2-D f32 plans whose two passes both have specialised kernels: the row pass
// butterflies row pairs on its input, the column pass transforms half tiles of N/2 rows and twice the width (dct_spec.h,
// ColHalfSpec).  REDFT10 along the columns runs row pass -> column pass (decimation in frequency), REDFT01 column pass ->
// row pass (decimation in time), whatever order the plain plan uses.  DSPFFT_NO_SPLIT=1 disables it; DSPFFT_FORCE_SPLIT=1
// applies it wherever the kernels exist (tests on small frames).
void build_split(dspfft_plan_s *pl)
{
	if (pl->f64 || pl->rank != 2 || pl->passes.size() != 2 || env_int("DSPFFT_NO_SPLIT") == 1) return;
	const Pass *R = nullptr, *Cc = nullptr;
	for (const Pass &P : pl->passes) {
		if (!P.has_spec || !P.hostloop.empty() || P.pa.sb2_in || P.pa.sb2_out) return;
		if (P.type == Pass::ROW) R = &P; else if (P.type == Pass::COL) Cc = &P;
	}
	if (!R || !Cc) return;
	const int N = Cc->pa.N, ca = Cc->axis, ra = R->axis;
	const bool force = env_int("DSPFFT_FORCE_SPLIT") == 1;
	if (N % 4) return;
	SpecInfo hs;
	if (!be_find_half_spec(N, Cc->pa.ninner, &hs)) return;
	// Used when the full-length tile fills a CU's LDS on its own (8K: 4320 rows x 8 floats = 138 KB, one workgroup per CU) and the
	// half tiles fit twice: measured 935 vs 1027 us per 7680x4320x3 roundtrip.  At 3840x2160 the half tiles are wider instead
	// (1080 x 16 floats, 64-B row segments: column passes 42-45 us instead of 46-49) but the paired row pass loses more than that
	// (2 rows per workgroup in sequence, 2 workgroups per CU: 52-55 us instead of 37-39) -- 58.3K vs 58.6K Mpix/s on two streams,
	// 41.4K vs 48.9K on one (tools/sbench.hip, tools/bench_8k_split.py; profiles/r02_split.txt) -- so 4K keeps the plain passes.
	// The half tile may also take the whole LDS again with twice the width (4320: 2160 rows x 16 floats): an 8K frame does not fit the
	// Infinity Cache, and HBM serves 64-byte row segments so much better than 32-byte ones that one workgroup per CU wins (882 vs 922 us).
	if (!force && !(Cc->spec.lds > 80 * 1024 && hs.lds <= Cc->spec.lds + 4096)) return;
	const int pid = be_find_row_pair(R->pa.N, R->pa.C);
	if (pid < 0) return;
	const bool col_first = pl->kinds[ca] == DSPFFT_REDFT01;
	std::vector<Pass> sp(2);
	Pass &PR = sp[col_first ? 1 : 0], &PC = sp[col_first ? 0 : 1];
	auto drop = [&]() { for (Pass &P : sp) P.tab.release(); };
	if (build_pass(pl, ra, !col_first, PR) || build_pass(pl, ca, col_first, PC)) { drop(); return; }
	// the row pass's first batch dimension must be the split axis, line for line
	const long long cis = col_first ? pl->axes[ca].os : pl->axes[ca].is, cos_ = pl->axes[ca].os;
	if (PR.type != Pass::ROW || !PR.has_spec || !PR.hostloop.empty() || PR.spa.nb0 != N || PR.spa.sb0_in != cis || PR.spa.sb0_out != cos_ ||
	    PC.type != Pass::COL || !PC.has_spec || !PC.hostloop.empty()) { drop(); return; }
	char buf[256];
	PR.pair = true; PR.pair_id = pid;
	snprintf(buf, sizeof buf, "axis %d: ROW*2 N=%d C=%d row pairs of axis %d, spec#%d threads=%d pairs=%d lds=%zu", ra, PR.pa.N, PR.pa.C, ca, PR.spec.id, be_row_pair_threads(pid), PR.spec_nwg / 2, PR.spec.lds);
	PR.desc = buf;
	// column pass: FFT of length N/2; T stays the table of the full length, W becomes the half length's, H = exp(-2 pi i n / N)
	const int M = N / 2;
	{
		const long double pi = 3.14159265358979323846264338327950288L;
		std::vector<cf> W(M), H(M);
		for (int t = 0; t < M; t++) { W[t] = cmk<float>((float)cosl(2 * pi * t / M), (float)-sinl(2 * pi * t / M)); H[t] = cmk<float>((float)cosl(2 * pi * t / N), (float)-sinl(2 * pi * t / N)); }
		be_free(PC.tab.W);
		PC.tab.W = be_alloc(W.size() * sizeof(cf)); PC.tab.H = be_alloc(H.size() * sizeof(cf));
		if (!PC.tab.W || !PC.tab.H || be_upload(PC.tab.W, W.data(), W.size() * sizeof(cf)) || be_upload(PC.tab.H, H.data(), H.size() * sizeof(cf))) { drop(); return; }
	}
	PC.half = true; PC.hspec = hs; PC.hpa = PC.spa;
	PC.hpa.K = hs.P; PC.hpa.B = hs.P / 2; PC.hpa.ntiles = PC.pa.ninner / hs.P;
	PC.half_nwg = 2 * PC.hpa.ntiles * PC.pa.nb0 * PC.pa.nb1;
	snprintf(buf, sizeof buf, "axis %d: COL*/2 N=%d as 2 x %d, K=%d half#%d threads=%d inner=%d tiles=%d wgs=%d lds=%zu", ca, N, M, hs.P, hs.id, hs.nthr, PC.pa.ninner, 2 * PC.hpa.ntiles, PC.half_nwg, hs.lds);
	PC.desc = buf;
	pl->split = std::move(sp);
	pl->split_col_axis = ca;
}

// which pass list an execution uses: the split one unless the buffers or the plan's per-index scales rule it out
// Blocks of 4, 8 or 16 samples a side (motion's --blocksize 8x8x8 and the like): one pass over the data instead of one per axis
// (block_core.h).  Needs the x axis contiguous, a batch dimension to take a workgroup's blocks from (the blocks of a row of blocks in
// a [D][H][W] volume, or whole blocks of a block-major stack) and 16-byte aligned strides.
void build_block(dspfft_plan_s *pl)
{
	if (pl->f64 || pl->rank < 2 || env_int("DSPFFT_NO_BLOCK") == 1) return;
	for (const Pass &P : pl->passes) if (P.type != Pass::TINY || !P.hostloop.empty()) return;
	for (int a = 1; a < pl->rank; a++) if (pl->kinds[a] != pl->kinds[0]) return;
	int ax = -1;
	for (int a = 0; a < pl->rank; a++) if (pl->axes[a].is == 1 && pl->axes[a].os == 1) ax = a;
	if (ax < 0) return;
	std::vector<int> rest;
	for (int a = 0; a < pl->rank; a++) if (a != ax) rest.push_back(a);
	std::sort(rest.begin(), rest.end(), [&](int p, int q) { return pl->axes[p].is < pl->axes[q].is; });
	const int ay = rest[0], az = rest.size() > 1 ? rest[1] : -1;
	const int nx = pl->n[ax], ny = pl->n[ay], nz = az >= 0 ? pl->n[az] : 1;
	if (!be_block_supported(nx, ny, nz)) return;
	// the dimension a workgroup takes its G blocks from: the batch dimension of smallest stride
	std::vector<Dim> dims;
	for (const Dim &b : pl->batches) if (b.n > 1) dims.push_back(b);
	if (dims.empty()) return;
	size_t gi = 0;
	for (size_t i = 1; i < dims.size(); i++) if (dims[i].is < dims[gi].is) gi = i;
	const Dim grp = dims[gi];
	dims.erase(dims.begin() + gi);
	merge_dims(dims);
	if (dims.size() > BLOCK_MAX_DIMS) return;
	bool aligned = grp.is % 4 == 0 && grp.os % 4 == 0 && pl->axes[ay].is % 4 == 0 && pl->axes[ay].os % 4 == 0 &&
	               (az < 0 || (pl->axes[az].is % 4 == 0 && pl->axes[az].os % 4 == 0));
	long long nrest = 1;
	for (const Dim &d : dims) { aligned = aligned && d.is % 4 == 0 && d.os % 4 == 0; nrest *= d.n; }
	if (!aligned) return;
	BlockGeom &g = pl->blk;
	memset(&g, 0, sizeof g);
	g.nx = nx; g.ny = ny; g.nz = nz; pl->blk_kind = pl->kinds[0] == DSPFFT_REDFT10 ? KIND_REDFT10 : KIND_REDFT01;
	g.sy_in = pl->axes[ay].is; g.sy_out = pl->axes[ay].os; g.sz_in = az >= 0 ? pl->axes[az].is : 0; g.sz_out = az >= 0 ? pl->axes[az].os : 0;
	g.sxb_in = grp.is; g.sxb_out = grp.os;
	g.rows_fast = !(grp.is == nx && grp.os == nx);
	// tiles of about 4096 samples = 16 KB (measured on 1920x1080x256, tools/bench_blocks.py: 8x8x8 blocks 2.44 ms per roundtrip with 64 KB
	// tiles, 1.77 ms with 16 KB ones -- eight and more workgroups per CU), rows of at most 1 KB
	int G = std::min(256 / nx, 4096 / (nx * ny * nz));
	if (env_int("DSPFFT_BLOCK_G")) G = env_int("DSPFFT_BLOCK_G");      // experiments (tools/bench_blocks.py)
	G = std::max(1, std::min(G, grp.n));
	if ((size_t)nz * ny * G * nx * sizeof(float) > 64 * 1024) return;
	g.G = G; g.nxb = grp.n; g.ngroups = (grp.n + G - 1) / G; g.pitch = G * nx; g.gdiv = make_div((uint32_t)g.ngroups);
	g.nd = (int)dims.size();
	for (int d = 0; d < g.nd; d++) { g.bn[d] = dims[d].n; g.bis[d] = dims[d].is; g.bos[d] = dims[d].os; g.bdiv[d] = make_div((uint32_t)dims[d].n); }
	const long long nwg = (long long)g.ngroups * nrest;
	if (nwg > 0x7fffffffLL) return;
	pl->blk_nwg = (int)nwg; pl->blk_lds = (size_t)nz * ny * g.pitch * sizeof(float);
	pl->blk_axis[0] = ax; pl->blk_axis[1] = ay; pl->blk_axis[2] = az;
	char buf[256];
	snprintf(buf, sizeof buf, "axes %d,%d%s: BLOCK %dx%dx%d (x,y,z) all axes in one pass, %d blocks per workgroup (%s), wgs=%d lds=%zu",
	         ax, ay, az >= 0 ? (std::string(",") + std::to_string(az)).c_str() : "", nx, ny, nz, G, g.rows_fast ? "block-major" : "side by side along x", pl->blk_nwg, pl->blk_lds);
	pl->blk_desc = buf;
	pl->has_block = true;
}

void block_scales(const dspfft_plan_s *pl, BlockScales &s)
{
	s.scale = (float)pl->scale;
	for (int i = 0; i < 3; i++) { const int ax = pl->blk_axis[i]; s.in0[i] = ax >= 0 ? (float)pl->in0[ax] : 1.f; s.out0[i] = ax >= 0 ? (float)pl->out0[ax] : 1.f; }
}

int run_block(const dspfft_plan_s *pl, const float *in, float *out, void *stream)
{
	BlockArgs a;
	static_cast<BlockGeom &>(a) = pl->blk;
	a.kind = pl->blk_kind; a.in = in; a.out = out;
	block_scales(pl, a.s);
	if (int rc = be_launch_block(a, pl->blk_nwg, pl->blk_lds, stream)) return fail(-4, "kernel launch failed (%s): backend code %d", pl->blk_desc.c_str(), rc);
	return 0;
}

// motion's per-block pipeline as one pass (block_core.h): both plans fuse their blocks the same way
bool block_roundtrip_ok(const dspfft_plan_s *f, const dspfft_plan_s *i)
{
	if (!f->has_block || !i->has_block || f->blk_kind != KIND_REDFT10 || i->blk_kind != KIND_REDFT01) return false;
	const BlockGeom &a = f->blk, &b = i->blk;
	bool ok = a.nx == b.nx && a.ny == b.ny && a.nz == b.nz && a.G == b.G && a.nxb == b.nxb && a.nd == b.nd && a.rows_fast == b.rows_fast &&
	          a.sy_out == b.sy_in && a.sz_out == b.sz_in && a.sxb_out == b.sxb_in && f->blk_nwg == i->blk_nwg;
	for (int k = 0; k < 3; k++) ok = ok && f->blk_axis[k] == i->blk_axis[k];
	for (int d = 0; ok && d < a.nd; d++) ok = a.bn[d] == b.bn[d] && a.bos[d] == b.bis[d];
	return ok;
}

const std::vector<Pass> &pick_passes(const dspfft_plan_s *pl, const void *in, const void *out)
{
	if (pl->split.empty()) return pl->passes;
	if (15u & ((uintptr_t)in | (uintptr_t)out)) return pl->passes;
	const int ca = pl->split_col_axis;
	// the row-pair butterfly mixes index 0 of the split axis with index N-1: scales on that index need the plain passes
	if (pl->kinds[ca] == DSPFFT_REDFT10 ? pl->in0[ca] != 1.0 : pl->out0[ca] != 1.0) return pl->passes;
	return pl->split;
}
}  // namespace

static int plan_finish(dspfft_plan_s *pl, dspfft_plan *plan, bool first_axis_first)
{
	EnvScope env;                 // the planner's switches, read once for this plan
	pl->plan_effort = g_plan_effort;
	memcpy(pl->plan_env, env.v, sizeof env.v);
	size_t samples = 1;
	pl->howmany = 1;
	for (const Dim &b : pl->batches) { samples *= (size_t)b.n; pl->howmany *= b.n; }
	for (int a = 0; a < pl->rank; a++) samples *= (size_t)pl->n[a];
	pl->alg_bytes = samples * (pl->f64 ? 16 : 8);
	pl->first_axis_first = first_axis_first;
	bool first = true;
	for (int i = 0; i < pl->rank; i++) {
		const int a = first_axis_first ? i : pl->rank - 1 - i;
		pl->passes.emplace_back();
		int rc = build_pass(pl, a, first, pl->passes.back());
		if (rc) { dspfft_destroy_plan(pl); return rc; }
		first = false;
	}
	build_split(pl);
	build_block(pl);
	*plan = pl;
	return 0;
}

static int plan_many(dspfft_plan *plan, int rank, const int *n, int howmany,
                     const int *inembed, int istride, int idist,
                     const int *onembed, int ostride, int odist, const int *kinds, bool f64, bool first_axis_first = false)
{
	if (!plan) return fail(-1, "null plan pointer");
	*plan = nullptr;
	if (rank < 1 || rank > 3) return fail(-1, "rank %d unsupported (1..3)", rank);
	if (howmany < 1 || istride < 1 || ostride < 1) return fail(-1, "howmany/stride must be >= 1");
	for (int a = 0; a < rank; a++) {
		if (n[a] < 1) return fail(-1, "n[%d] = %d", a, n[a]);
		if (kinds[a] != DSPFFT_REDFT10 && kinds[a] != DSPFFT_REDFT01) return fail(-1, "kind %d unsupported (REDFT10/REDFT01 only)", kinds[a]);
		if ((inembed && inembed[a] < n[a] && a > 0) || (onembed && onembed[a] < n[a] && a > 0)) return fail(-1, "embed smaller than n");
	}
	dspfft_plan_s *pl = new dspfft_plan_s();
	pl->rank = rank; pl->scale = 1.0; pl->f64 = f64;
	long long is = istride, os = ostride;
	for (int a = rank - 1; a >= 0; a--) {
		pl->n[a] = n[a]; pl->kinds[a] = kinds[a]; pl->in0[a] = pl->out0[a] = 1.0;
		pl->axes[a].n = n[a]; pl->axes[a].is = is; pl->axes[a].os = os;
		is *= inembed ? inembed[a] : n[a]; os *= onembed ? onembed[a] : n[a];
	}
	if (howmany > 1) pl->batches.push_back(Dim{howmany, idist, odist});
	return plan_finish(pl, plan, first_axis_first);
}

extern "C" int dspfft_plan_many_r2r(dspfft_plan *plan, int rank, const int *n, int howmany,
                                    const int *inembed, int istride, int idist,
                                    const int *onembed, int ostride, int odist, const int *kinds)
{
	return plan_many(plan, rank, n, howmany, inembed, istride, idist, onembed, ostride, odist, kinds, false);
}
extern "C" int dspfft_plan_many_r2r_f64(dspfft_plan *plan, int rank, const int *n, int howmany,
                                        const int *inembed, int istride, int idist,
                                        const int *onembed, int ostride, int odist, const int *kinds)
{
	return plan_many(plan, rank, n, howmany, inembed, istride, idist, onembed, ostride, odist, kinds, true);
}

// FFTW's guru interface shape (fftw_plan_guru_r2r): every transformed and every batch dimension has its own extent and
// input / output strides, so e.g. all 8x8x8 blocks of a volume (motion --blocksize 8x8x8) are ONE plan
static int plan_guru(dspfft_plan *plan, int rank, const dspfft_iodim *dims, int howmany_rank, const dspfft_iodim *howmany_dims, const int *kinds, int f64,
                     bool first_axis_first)
{
	if (!plan) return fail(-1, "null plan pointer");
	*plan = nullptr;
	if (rank < 1 || rank > 3 || !dims || !kinds) return fail(-1, "rank %d unsupported (1..3)", rank);
	if (howmany_rank < 0 || howmany_rank > 6 || (howmany_rank && !howmany_dims)) return fail(-1, "howmany_rank %d unsupported (0..6)", howmany_rank);
	for (int a = 0; a < rank; a++) {
		if (dims[a].n < 1 || dims[a].is < 1 || dims[a].os < 1) return fail(-1, "dims[%d] must have n, is, os >= 1", a);
		if (kinds[a] != DSPFFT_REDFT10 && kinds[a] != DSPFFT_REDFT01) return fail(-1, "kind %d unsupported (REDFT10/REDFT01 only)", kinds[a]);
	}
	for (int b = 0; b < howmany_rank; b++)
		if (howmany_dims[b].n < 1 || howmany_dims[b].is < 0 || howmany_dims[b].os < 0) return fail(-1, "howmany_dims[%d] must have n >= 1 and non-negative strides", b);
	dspfft_plan_s *pl = new dspfft_plan_s();
	pl->rank = rank; pl->scale = 1.0; pl->f64 = f64 != 0;
	for (int a = 0; a < rank; a++) {
		pl->n[a] = dims[a].n; pl->kinds[a] = kinds[a]; pl->in0[a] = pl->out0[a] = 1.0;
		pl->axes[a].n = dims[a].n; pl->axes[a].is = dims[a].is; pl->axes[a].os = dims[a].os;
	}
	for (int b = 0; b < howmany_rank; b++) if (howmany_dims[b].n > 1) pl->batches.push_back(Dim{howmany_dims[b].n, howmany_dims[b].is, howmany_dims[b].os});
	return plan_finish(pl, plan, first_axis_first);
}
extern "C" int dspfft_plan_guru_r2r(dspfft_plan *plan, int rank, const dspfft_iodim *dims, int howmany_rank, const dspfft_iodim *howmany_dims,
                                    const int *kinds, int f64)
{
	return plan_guru(plan, rank, dims, howmany_rank, howmany_dims, kinds, f64, false);
}
// ... with the pass order of dspfft_plan_many_r2r_ordered (f32): first_axis_first runs axis 0 first and the last axis last
extern "C" int dspfft_plan_guru_r2r_ordered(dspfft_plan *plan, int rank, const dspfft_iodim *dims, int howmany_rank, const dspfft_iodim *howmany_dims,
                                            const int *kinds, int first_axis_first)
{
	return plan_guru(plan, rank, dims, howmany_rank, howmany_dims, kinds, 0, first_axis_first != 0);
}

extern "C" int dspfft_plan_many_r2r_ordered(dspfft_plan *plan, int rank, const int *n, int howmany,
                                            const int *inembed, int istride, int idist,
                                            const int *onembed, int ostride, int odist, const int *kinds, int first_axis_first)
{
	return plan_many(plan, rank, n, howmany, inembed, istride, idist, onembed, ostride, odist, kinds, false, first_axis_first != 0);
}

extern "C" int dspfft_plan_r2r_2d(dspfft_plan *plan, int n0, int n1, int kind0, int kind1)
{
	int n[2] = {n0, n1}, k[2] = {kind0, kind1};
	return dspfft_plan_many_r2r(plan, 2, n, 1, nullptr, 1, 0, nullptr, 1, 0, k);
}

extern "C" int dspfft_plan_set_scale(dspfft_plan pl, float scale)
{
	if (!pl) return fail(-1, "null plan");
	pl->scale = scale; return 0;
}
extern "C" int dspfft_plan_set_axis_scale0(dspfft_plan pl, int axis, float in_scale0, float out_scale0)
{
	if (!pl || axis < 0 || axis >= pl->rank) return fail(-1, "bad plan/axis");
	pl->in0[axis] = in_scale0; pl->out0[axis] = out_scale0; return 0;
}
// Input rows of `axis` outside [lo, hi) are zero by contract and need not be read.  Honoured (return 1) only where it is implemented:
// f32 plans whose FIRST pass is a listed specialised column REDFT01 pass along `axis` (zoom's y stage); returns 0 -- nothing changes, the
// caller must really store those zeros -- everywhere else.  lo = hi = 0 turns it off.
extern "C" int dspfft_plan_set_input_window(dspfft_plan pl, int axis, int lo, int hi)
{
	if (!pl || axis < 0 || axis >= pl->rank || lo < 0 || hi < lo || hi > pl->n[axis]) return fail(-1, "bad plan / axis / window");
	pl->win_axis = -1; pl->win_lo = pl->win_hi = 0;
	pl->mod_axis = -1; pl->mod_table = nullptr; pl->mod_rev = 0;      // a modulation lives on its window
	if (hi == 0) return 0;
	if (pl->f64 || pl->passes.empty() || !pl->split.empty() || pl->has_block) return 0;
	const Pass &P = pl->passes[0];
	if (P.axis != axis || (P.type != Pass::COL && P.type != Pass::ROW) || !P.has_spec || P.jit || pl->kinds[axis] != DSPFFT_REDFT01 || !P.hostloop.empty()) return 0;
	if (!pl->zpage) { pl->zpage = be_alloc(64); if (pl->zpage) { const char z[64] = {0}; if (be_upload(pl->zpage, z, 64)) { be_free(pl->zpage); pl->zpage = nullptr; } } }
	if (!pl->zpage) return 0;
	pl->win_axis = axis; pl->win_lo = lo; pl->win_hi = hi;
	return 1;
}
// Input sample x of `axis` is read from position p = reversed_from > 0 ? reversed_from - x : x of its line and multiplied by d_mul[p]
// (floats, device memory, kept by the caller) as it is loaded.  Only together with an input window (set it first): samples outside the
// window stay zero, and with reversed_from every sample inside it must map to a position >= 0.  Honoured (return 1) for f32 plans whose
// FIRST pass is a listed specialised ROW or COL REDFT01 pass along `axis`; d_mul = NULL turns it off.
extern "C" int dspfft_plan_set_input_modulation(dspfft_plan pl, int axis, const float *d_mul, int reversed_from)
{
	if (!pl || axis < 0 || axis >= pl->rank || reversed_from < 0) return fail(-1, "bad plan / axis / reversal");
	pl->mod_axis = -1; pl->mod_table = nullptr; pl->mod_rev = 0;
	if (!d_mul) return 0;
	if (pl->win_axis != axis || pl->win_hi <= 0) return 0;
	if (reversed_from > 0 && pl->win_hi - 1 > reversed_from) return fail(-1, "input window [%d, %d) reaches beyond the reversal point %d", pl->win_lo, pl->win_hi, reversed_from);
	if (pl->passes.empty() || (pl->passes[0].type != Pass::ROW && pl->passes[0].type != Pass::COL)) return 0;
	pl->mod_axis = axis; pl->mod_table = d_mul; pl->mod_rev = reversed_from;
	return 1;
}
// Output sample j of `axis` times (-1)^j, fused into the pass of that axis.  Honoured (return 1) only where it is implemented: f32 plans
// whose pass along `axis` is a listed specialised column or row REDFT01 pass and the plan's LAST one; 0 otherwise (nothing changes).
extern "C" int dspfft_plan_set_output_alternate(dspfft_plan pl, int axis, int on)
{
	if (!pl || axis < 0 || axis >= pl->rank) return fail(-1, "bad plan / axis");
	pl->alt_axis = -1;
	if (!on) return 0;
	if (pl->f64 || pl->passes.empty() || !pl->split.empty() || pl->has_block) return 0;
	const Pass &P = pl->passes.back();
	if (P.axis != axis || (P.type != Pass::COL && P.type != Pass::ROW) || !P.has_spec || P.jit || pl->kinds[axis] != DSPFFT_REDFT01 || !P.hostloop.empty()) return 0;
	pl->alt_axis = axis;
	return 1;
}
extern "C" int dspfft_plan_set_scale_f64(dspfft_plan pl, double scale)
{
	if (!pl) return fail(-1, "null plan");
	pl->scale = scale; return 0;
}
extern "C" int dspfft_plan_set_axis_scale0_f64(dspfft_plan pl, int axis, double in_scale0, double out_scale0)
{
	if (!pl || axis < 0 || axis >= pl->rank) return fail(-1, "bad plan/axis");
	pl->in0[axis] = in_scale0; pl->out0[axis] = out_scale0; return 0;
}

namespace {
template <class R>
int execute_t(dspfft_plan pl, const R *d_in, R *d_out, void *stream)
{
	if (!pl || !d_in || !d_out) return fail(-1, "null plan or buffer");
	if (pl->f64 != std::is_same<R, double>::value) return fail(-1, "plan and buffers differ in sample type (f32 plan <-> dspfft_execute, f64 plan <-> dspfft_execute_f64)");
	if constexpr (std::is_same<R, float>::value) {
		if (pl->has_block && !(15u & ((uintptr_t)d_in | (uintptr_t)d_out))) return run_block(pl, d_in, d_out, stream);
	}
	const std::vector<Pass> &passes = pick_passes(pl, d_in, d_out);
	for (size_t i = 0; i < passes.size(); i++) {
		const Pass &P = passes[i];
		int rc = run_pass<R>(pl, P, P.first ? d_in : d_out, d_out, i + 1 == passes.size(), stream);
		if (rc) return rc;
	}
	return 0;
}
template <class R>
int execute_masked_accumulate_t(dspfft_plan pl, const R *d_in, R *d_work, R *d_acc, const uint32_t *d_ids, uint32_t lo, uint32_t span, int elems_per_id, void *stream);
}  // namespace

extern "C" int dspfft_execute(dspfft_plan pl, const float *d_in, float *d_out, void *stream) { return execute_t<float>(pl, d_in, d_out, stream); }
extern "C" int dspfft_execute_f64(dspfft_plan pl, const double *d_in, double *d_out, void *stream) { return execute_t<double>(pl, d_in, d_out, stream); }
extern "C" int dspfft_execute_masked_accumulate(dspfft_plan pl, const float *d_in, float *d_work, float *d_acc,
                                                const uint32_t *d_ids, uint32_t id, int elems_per_id, void *stream)
{
	return execute_masked_accumulate_t<float>(pl, d_in, d_work, d_acc, d_ids, id, 1, elems_per_id, stream);
}
extern "C" int dspfft_execute_masked_accumulate_f64(dspfft_plan pl, const double *d_in, double *d_work, double *d_acc,
                                                    const uint32_t *d_ids, uint32_t id, int elems_per_id, void *stream)
{
	return execute_masked_accumulate_t<double>(pl, d_in, d_work, d_acc, d_ids, id, 1, elems_per_id, stream);
}
// [lo, hi) as (lo, span): hi <= 0xFFFFFFFF keeps the DC pixel's 0xFFFFFFFF out of every range (mask_pick); hi <= lo selects nothing
extern "C" int dspfft_execute_masked_accumulate_range(dspfft_plan pl, const float *d_in, float *d_work, float *d_acc,
                                                      const uint32_t *d_ids, uint32_t lo, uint32_t hi, int elems_per_id, void *stream)
{
	if (!d_ids) return fail(-1, "dspfft_execute_masked_accumulate_range needs an owner-id array");
	return execute_masked_accumulate_t<float>(pl, d_in, d_work, d_acc, d_ids, lo, hi > lo ? hi - lo : 0, elems_per_id, stream);
}
extern "C" int dspfft_execute_masked_accumulate_range_f64(dspfft_plan pl, const double *d_in, double *d_work, double *d_acc,
                                                          const uint32_t *d_ids, uint32_t lo, uint32_t hi, int elems_per_id, void *stream)
{
	if (!d_ids) return fail(-1, "dspfft_execute_masked_accumulate_range_f64 needs an owner-id array");
	return execute_masked_accumulate_t<double>(pl, d_in, d_work, d_acc, d_ids, lo, hi > lo ? hi - lo : 0, elems_per_id, stream);
}

namespace {
// Sparse frames of the fused scan step: one image, a specialised column pass first and a specialised row pass over the same dense rows
// second.  The column pass flags the tiles none of whose coefficients belongs to the frame and leaves them alone; the row pass reads
// zeros there.  At BASELINE config 4 (zigzag, 32 frames) a frame touches about half of the columns.  The 1-D passes commute; a plain
// plan lists ROW before COL, and a frame of a wide image is sparser in columns than in rows, so the column pass goes first when input
// and output strides agree (a pass's geometry is built for its place in the list).  Returns false when the plan does not qualify.
bool sparse_order(const dspfft_plan_s *pl, const std::vector<Pass> &passes, bool split, size_t order[2])
{
	order[0] = 0; order[1] = 1;
	if (passes.size() != 2 || env_int("DSPFFT_NO_ZSKIP") == 1) return false;
	// measured (tools/bench_scan_step.py): 7680x4320x3 on the split passes 630 -> 513 us per frame; 3840x2160x3 on the plain passes
	// 119 -> 122 us (the frame lives in the Infinity Cache and the flag lookups cost what the skipped reads save), so plain plans
	// take part only on request (DSPFFT_ZSKIP=1: the tests of the mechanism on small frames)
	if (!split && env_int("DSPFFT_ZSKIP") != 1) return false;
	if (!split && passes[0].type == Pass::ROW && passes[1].type == Pass::COL) {
		bool same = true;
		for (int b = 0; b < pl->rank; b++) same = same && pl->axes[b].is == pl->axes[b].os;
		for (const Dim &b : pl->batches) same = same && b.is == b.os;
		if (same) { order[0] = 1; order[1] = 0; }
	}
	const Pass &PC = passes[order[0]], &PR = passes[order[1]];
	const bool col_ok = PC.type == Pass::COL && (split ? PC.half : PC.has_spec), row_ok = PR.type == Pass::ROW && (split ? PR.pair : PR.has_spec);
	const PassGeom &gc = split ? PC.hpa : PC.spa, &gr = PR.spa;
	const bool ok = col_ok && row_ok && PC.hostloop.empty() && PR.hostloop.empty() && !gr.sb2_in && !gr.sb2_out && gc.nb0 == 1 && gc.nb1 == 1 && gr.nb1 == 1 && gr.nb0 == gc.N &&
	                gr.N * gr.C == gc.ninner && gr.sb0_in == gc.ninner && gc.es_in == gc.ninner && gc.es_out == gc.ninner && gc.ninner % gc.K == 0 && (gc.K & (gc.K - 1)) == 0;
	if (!ok) { order[0] = 0; order[1] = 1; }
	return ok;
}
}  // namespace

extern "C" int dspfft_plan_scan_prepare(dspfft_plan pl, const uint32_t *d_ids, int elems_per_id, void *stream)
{
	if (!pl) return fail(-1, "null plan");
	pl->zr_ids = nullptr;                       // forget what was prepared before
	if (!d_ids) return 0;
	if (elems_per_id < 1) return fail(-1, "elems_per_id must be >= 1");
	const bool split = !pl->split.empty();
	const std::vector<Pass> &passes = split ? pl->split : pl->passes;
	size_t order[2];
	if (!sparse_order(pl, passes, split, order)) return 0;      // nothing to prepare for this plan: executes read every owner id
	const PassGeom &gc = split ? passes[order[0]].hpa : passes[order[0]].spa;
	const int halves = split ? 2 : 1;
	const size_t need = (size_t)2 * halves * gc.ntiles * sizeof(uint32_t);
	if (pl->zranges_bytes < need) { be_free(pl->zranges); pl->zranges = be_alloc(need); pl->zranges_bytes = pl->zranges ? need : 0; }
	if (!pl->zranges) return fail(-3, "allocation failed");
	TileRangeGeom g;
	g.K = gc.K; g.ntiles = gc.ntiles; g.nrows = gc.N / halves; g.row_start = 0; g.row_step = 1; g.es = gc.es_in; g.div = make_div((uint32_t)elems_per_id);
	if (be_scan_tile_ranges((uint32_t *)pl->zranges, d_ids, g, halves, stream)) return fail(-4, "launch failed");
	pl->zr_ids = d_ids; pl->zr_div = elems_per_id; pl->zr_split = split;
	// the element-order id table (dct_spec.h, masked_two_step): one byte per id while every frame id is below 255, else two.
	// DSPFFT_SCAN_EIDS=0: not built (A/B runs)
	pl->eid_bytes = 0;
	const char *env_eids = getenv("DSPFFT_SCAN_EIDS");
	const bool no_eids = env_eids && *env_eids == '0';
	if (!pl->f64 && !no_eids && gc.K % 4 == 0 && gc.es_in % elems_per_id == 0 && (long long)gc.ntiles * gc.K == gc.ninner) {
		std::vector<uint32_t> rg((size_t)2 * halves * gc.ntiles);
		if (be_download(rg.data(), pl->zranges, rg.size() * sizeof(uint32_t), stream)) return fail(-4, "download failed");
		uint32_t top = 0;
		for (size_t i = 0; i < rg.size(); i += 2) if (rg[i] <= rg[i + 1] && rg[i + 1] > top) top = rg[i + 1];      // (an empty tile holds lo > hi)
		const int eb = top < 0xffu ? 1 : top < 0xffffu ? 2 : 0;
		const size_t bytes = (size_t)gc.ntiles * gc.N * gc.K * eb;
		if (eb) {
			if (pl->eids_bytes < bytes) { be_free(pl->eids); pl->eids = be_alloc(bytes); pl->eids_bytes = pl->eids ? bytes : 0; }
			if (pl->eids) {
				TileEidGeom e;
				e.K = gc.K; e.ntiles = gc.ntiles; e.N = gc.N; e.halves = halves; e.bytes = eb; e.es = gc.es_in; e.div = make_div((uint32_t)elems_per_id);
				if (be_scan_tile_eids(pl->eids, d_ids, e, stream)) return fail(-4, "launch failed");
				pl->eid_bytes = eb;
			}
		}
	}
	return 0;
}

namespace {
template <class R>
int execute_masked_accumulate_t(dspfft_plan pl, const R *d_in, R *d_work, R *d_acc, const uint32_t *d_ids, uint32_t lo, uint32_t span, int elems_per_id, void *stream)
{
	if (!pl || !d_in || !d_work || !d_acc) return fail(-1, "null plan or buffer");
	if (pl->f64 != std::is_same<R, double>::value) return fail(-1, "plan and buffers differ in sample type");
	if (d_ids && elems_per_id < 1) return fail(-1, "elems_per_id must be >= 1");
	if (d_ids && (unsigned long long)pl->alg_bytes / (2 * sizeof(R)) * (unsigned)elems_per_id >= (1ull << 32))
		return fail(-2, "masked execution addresses elements with 32-bit offsets: plan too large");
	// the split passes (row pairs + half tiles) carry the mask and the accumulation like the plain ones: the row-pair butterfly
	// runs on the masked inputs, which is what masking the coefficients first means
	const bool split_ok = !pl->split.empty() && !(15u & ((uintptr_t)d_in | (uintptr_t)d_work | (uintptr_t)d_acc)) && &pick_passes(pl, d_in, d_acc) == &pl->split;
	const std::vector<Pass> &passes = split_ok ? pl->split : pl->passes;
	const size_t np = passes.size();
	for (const Pass &P : passes)
		if (!P.hostloop.empty() || P.pa.sb2_in || P.pa.sb2_out) return fail(-2, "masked/accumulating execution is not available for plans with more than two batch levels");
	// Sparse frames: one image, a specialised column pass first and a specialised row pass over the same dense rows second.  The
	// column pass flags the tiles none of whose coefficients belongs to this frame and leaves them alone; the row pass reads zeros
	// there.  At BASELINE config 4 (zigzag, 32 frames) a frame touches about half of the columns.
	uint8_t *zflags = nullptr;
	int zshift = 0, zhalf = 0;
	const uint32_t *zranges = nullptr;
	const void *eids = nullptr;
	int eid_bytes = 0;
	size_t order[2] = {0, 1};
	if (d_ids && np == 2 && sparse_order(pl, passes, split_ok, order)) {
		const PassGeom &gc = split_ok ? passes[order[0]].hpa : passes[order[0]].spa;
		const size_t al = sizeof(R) * 4;
		if (!((al - 1) & ((uintptr_t)d_in | (uintptr_t)d_work | (uintptr_t)d_acc))) {
			const size_t need = (size_t)2 * gc.ntiles;
			if (pl->zflags_bytes < need) { be_free(pl->zflags); pl->zflags = be_alloc(need); pl->zflags_bytes = pl->zflags ? need : 0; }
			if (!pl->zpage) { pl->zpage = be_alloc(64); if (pl->zpage) { const char z[64] = {0}; if (be_upload(pl->zpage, z, 64)) { be_free(pl->zpage); pl->zpage = nullptr; } } }
			if (pl->zflags && pl->zpage) {
				zflags = (uint8_t *)pl->zflags; zhalf = split_ok ? gc.ntiles : 0;
				while ((1 << zshift) < gc.K) zshift++;
				if (pl->zranges && pl->zr_ids == (const void *)d_ids && pl->zr_div == elems_per_id && pl->zr_split == split_ok) {
					// the (min, max) tile skip compares one frame id (the column launchers' test, which the CPU emulation of the kernels repeats);
					// a range of several ids reads the tiles' ids and still skips the tiles that selected nothing
					zranges = span == 1 ? (const uint32_t *)pl->zranges : nullptr;
					if (pl->eid_bytes) { eids = pl->eids; eid_bytes = pl->eid_bytes; }
				}
			}
		}
	}
	if (!zflags) { order[0] = 0; order[1] = 1; }
	for (size_t i = 0; i < np; i++) {
		const Pass &P = passes[np == 2 ? order[i] : i];
		const bool firstp = i == 0, lastp = i + 1 == np;
		Fuse fz;
		if (firstp && d_ids) { fz.mask = d_ids; fz.id = lo; fz.span = span; fz.div = elems_per_id; }
		fz.accumulate = lastp;
		fz.zflags = zflags; fz.zshift = zshift; fz.zhalf = zhalf; fz.zpage = pl->zpage; fz.zranges = zranges;
		if (firstp && std::is_same<R, float>::value) { fz.eids = eids; fz.eid_bytes = eid_bytes; }
		const R *src = firstp ? d_in : d_work;
		R *dst = lastp ? d_acc : d_work;
		int rc = run_pass<R>(pl, P, src, dst, lastp, stream, fz);
		if (rc) return rc;
	}
	return 0;
}
}  // namespace

// out = a(in_a) + b(in_b).  One launch when both are f32 single-pass plans on the same listed row REDFT01 kernel writing the same lines
// (zoom's x stage: the cosine and the sine part of a shifted cosine series); otherwise a's execution followed by b's accumulating one.
extern "C" int dspfft_execute_sum2(dspfft_plan pa, dspfft_plan pb, const float *d_in_a, const float *d_in_b, float *d_out, void *stream)
{
	if (!pa || !pb || !d_in_a || !d_in_b || !d_out) return fail(-1, "null plan or buffer");
	if (pa->f64 || pb->f64) return fail(-1, "dspfft_execute_sum2 takes f32 plans");
	auto one_row = [](const dspfft_plan_s *pl) {
		if (pl->passes.size() != 1 || !pl->split.empty() || pl->has_block) return false;
		const Pass &P = pl->passes[0];
		return P.type == Pass::ROW && P.has_spec && !P.jit && P.hostloop.empty() && !P.pa.sb2_in && !P.pa.sb2_out && pl->kinds[P.axis] == DSPFFT_REDFT01;
	};
	if (one_row(pa) && one_row(pb)) {
		const Pass &A = pa->passes[0], &B = pb->passes[0];
		const PassGeom &ga = A.spa, &gb = B.spa;
		if (A.spec.id == B.spec.id && A.spec_nwg == B.spec_nwg && ga.nb0 == gb.nb0 && ga.nb1 == gb.nb1 && ga.sb0_out == gb.sb0_out && ga.sb1_out == gb.sb1_out) {
			// same pointer rule as run_pass (whole pixels per access); the two-launch path below applies it by itself
			const uintptr_t al = sizeof(float) * (ga.C == 2 || ga.C == 4 ? ga.C : 1);
			if ((al - 1) & ((uintptr_t)d_in_a | (uintptr_t)d_in_b | (uintptr_t)d_out)) return fail(-1, "dspfft_execute_sum2: buffers must be aligned to a pixel of %d floats", ga.C);
			PassArgs a, b;
			fill_args(a, ga, pa, A, d_in_a, d_out, pa->scale, Fuse());
			fill_args(b, gb, pb, B, d_in_b, d_out, pb->scale, Fuse());
			if (int rc = be_launch_row_sum2(A.spec.id, a, b, A.spec_nwg, stream)) return fail(-4, "kernel launch failed (%s, sum of two): backend code %d", A.desc.c_str(), rc);
			return 0;
		}
	}
	// one after the other: b's accumulating execution has no work buffer of its own here, so b must be a one-pass plan
	if (pb->passes.size() != 1 || pb->has_block) return fail(-2, "dspfft_execute_sum2: the second plan must be a one-pass plan (its result is added in that pass's store)");
	if (int rc = dspfft_execute(pa, d_in_a, d_out, stream)) return rc;
	return dspfft_execute_masked_accumulate(pb, d_in_b, d_out, d_out, nullptr, 0, 1, stream);
}

// ---- rows of a phase-shifted cosine series (include/dspfft.h dspfft_cosrows_*; dct_duo.h) ----
struct dspfft_cosrows_s {
	int M, cw, vw, lines, id, nsrc;
	void *W;        // exp(-2 pi i t / (M/2)), t < M/2
	float *tab;     // [nsrc][M/2] slots of four floats, rebuilt per execution
};
extern "C" int dspfft_cosrows_create(dspfft_cosrows *out, int M, int cw, int vw, int lines)
{
	if (!out) return fail(-1, "null plan pointer");
	*out = nullptr;
	if (M < 4 || cw < 1 || cw > M || vw < 1 || vw > M || lines < 1) return fail(-1, "bad arguments (M %d, cw %d, vw %d, lines %d)", M, cw, vw, lines);
	const int id = be_find_zoomx(M);
	if (id < 0) return fail(-2, "no cosine-series row kernel for lines of %d samples", M);
	dspfft_cosrows p = new dspfft_cosrows_s();
	p->M = M; p->cw = cw; p->vw = vw; p->lines = lines; p->id = id;
	p->nsrc = 4 * cw <= M ? 1 : 2 * cw <= M ? 2 : 4;
	const int L = M / 2;
	std::vector<cf> w((size_t)L);
	const long double pi = 3.14159265358979323846264338327950288L;
	for (int t = 0; t < L; t++) w[t] = cmk<float>((float)cosl(2 * pi * t / L), (float)-sinl(2 * pi * t / L));
	p->W = be_alloc((size_t)L * sizeof(cf));
	p->tab = (float *)be_alloc((size_t)p->nsrc * L * 4 * sizeof(float));
	if (!p->W || !p->tab || be_upload(p->W, w.data(), w.size() * sizeof(cf))) {
		if (p->W) be_free(p->W);
		if (p->tab) be_free(p->tab);
		delete p;
		return fail(-3, "no device memory for the tables");
	}
	*out = p;
	return 0;
}
extern "C" int dspfft_cosrows_execute(dspfft_cosrows p, const float *d_in, long long in_pitch, float *d_out, long long out_pitch, double theta, double scale, void *stream)
{
	if (!p || !d_in || !d_out) return fail(-1, "null plan or buffer");
	if (in_pitch < 0 || out_pitch < 0 || (p->lines > 1 && (in_pitch < (long long)p->cw * 3 || out_pitch < (long long)p->vw * 3))) return fail(-1, "line pitch shorter than a line");
	if (3u & ((uintptr_t)d_in | (uintptr_t)d_out)) return fail(-1, "buffers must be 4-byte aligned");
	// 32-bit offsets inside a line
	if ((long long)p->M * 3 >= (1ll << 30)) return fail(-2, "line too long");
	if (int rc = be_zoomx_tables(p->tab, p->M, p->cw, p->nsrc, theta, scale, stream)) return fail(-4, "table kernel launch failed: backend code %d", rc);
	ZoomXArgs a;
	a.in = d_in; a.out = d_out; a.tab = p->tab; a.W = (const cf *)p->W; a.in_pitch = in_pitch; a.out_pitch = out_pitch; a.cw = p->cw; a.vw = p->vw; a.lines = p->lines;
	if (int rc = be_launch_zoomx(p->id, a, p->nsrc, p->vw < p->M, stream)) return fail(-4, "kernel launch failed (cosine-series rows, M = %d): backend code %d", p->M, rc);
	return 0;
}
extern "C" void dspfft_cosrows_destroy(dspfft_cosrows p)
{
	if (!p) return;
	be_free(p->W); be_free(p->tab);
	delete p;
}

// ---- chirp-z rows (include/dspfft.h dspfft_cztrows_*; dct_czt.h) ----
struct dspfft_cztrows_s {
	int nc, nout, lines, group, id, P;
	void *W;                    // exp(-2 pi i t / P)
	cf *atab, *etab, *htab, *hspec;
	double omega_of_spectrum;   // the omega hspec was made for (NaN: none yet)
};
extern "C" int dspfft_cztrows_create(dspfft_cztrows *out, int nc, int nout, int lines, int group)
{
	if (!out) return fail(-1, "null plan pointer");
	*out = nullptr;
	if (nc < 1 || nout < 1 || lines < 1 || group < 1 || lines % group) return fail(-1, "bad arguments (nc %d, nout %d, lines %d, group %d)", nc, nout, lines, group);
	int P = 0;
	const int id = be_find_czt(nc + nout - 1, &P);
	if (id < 0) return fail(-2, "no chirp-z row kernel for a convolution of %d points", nc + nout - 1);
	dspfft_cztrows p = new dspfft_cztrows_s();
	p->nc = nc; p->nout = nout; p->lines = lines; p->group = group; p->id = id; p->P = P;
	p->omega_of_spectrum = std::nan("");
	std::vector<cf> w((size_t)P);
	const long double pi = 3.14159265358979323846264338327950288L;
	for (int t = 0; t < P; t++) w[t] = cmk<float>((float)cosl(2 * pi * t / P), (float)-sinl(2 * pi * t / P));
	p->W = be_alloc((size_t)P * sizeof(cf));
	p->atab = (cf *)be_alloc(((size_t)nc + nout + 2 * (size_t)P) * sizeof(cf));
	if (!p->W || !p->atab || be_upload(p->W, w.data(), w.size() * sizeof(cf))) {
		if (p->W) be_free(p->W);
		if (p->atab) be_free(p->atab);
		delete p;
		return fail(-3, "no device memory for the tables");
	}
	p->etab = p->atab + nc; p->htab = p->etab + nout; p->hspec = p->htab + P;
	*out = p;
	return 0;
}
extern "C" int dspfft_cztrows_length(dspfft_cztrows p) { return p ? p->P : 0; }
extern "C" int dspfft_cztrows_execute_n(dspfft_cztrows p, int nc, int lines, const float *d_in, long long in_group, long long in_pitch, int es_in,
                                        float *d_out, long long out_group, long long out_pitch, int es_out, double omega, double phi, double scale, void *stream)
{
	if (!p || !d_in || !d_out || es_in < 1 || es_out < 1) return fail(-1, "null plan or buffer, or a stride below 1");
	if (nc < 1 || nc > p->nc || lines < 1 || lines > p->lines || lines % p->group)
		return fail(-1, "extents (nc %d, lines %d) outside the plan's (nc %d, lines %d, group %d)", nc, lines, p->nc, p->lines, p->group);
	if (3u & ((uintptr_t)d_in | (uintptr_t)d_out)) return fail(-1, "buffers must be 4-byte aligned");
	const bool fresh = !(omega == p->omega_of_spectrum);
	// the tables always for the plan's nc: the chirp's spectrum then serves every nc <= p->nc (a line of nc' components convolves with
	// h[m], m in (-(nc' - 1), nout), a sub-range of what it holds, and P >= p->nc + nout - 1 >= nc' + nout - 1); f0 reads only n < nc
	if (int rc = be_czt_tables(p->atab, p->etab, fresh ? p->htab : nullptr, p->nc, p->nout, p->P, omega, phi, scale, stream)) return fail(-4, "table kernel launch failed: backend code %d", rc);
	CztArgs a;
	a.in = nullptr; a.out = nullptr; a.atab = p->htab; a.hspec = nullptr; a.etab = nullptr; a.W = (const cf *)p->W;
	a.in_pitch = a.out_pitch = a.in_group = a.out_group = 0; a.es_in = a.es_out = 1; a.nc = p->P; a.nout = 0; a.lines = 1; a.group = 1;
	if (fresh) {
		if (int rc = be_launch_czt_spectrum(p->id, a, p->hspec, stream)) return fail(-4, "kernel launch failed (chirp spectrum, P = %d): backend code %d", p->P, rc);
		p->omega_of_spectrum = omega;
	}
	a.in = d_in; a.out = d_out; a.atab = p->atab; a.hspec = p->hspec; a.etab = p->etab;
	a.in_pitch = in_pitch; a.out_pitch = out_pitch; a.in_group = in_group; a.out_group = out_group; a.es_in = es_in; a.es_out = es_out;
	a.nc = nc; a.nout = p->nout; a.lines = lines; a.group = p->group;
	if (int rc = be_launch_czt_rows(p->id, a, stream)) return fail(-4, "kernel launch failed (chirp-z rows, P = %d): backend code %d", p->P, rc);
	return 0;
}
extern "C" int dspfft_cztrows_execute(dspfft_cztrows p, const float *d_in, long long in_group, long long in_pitch, int es_in,
                                      float *d_out, long long out_group, long long out_pitch, int es_out, double omega, double phi, double scale, void *stream)
{
	if (!p) return fail(-1, "null plan or buffer, or a stride below 1");
	return dspfft_cztrows_execute_n(p, p->nc, p->lines, d_in, in_group, in_pitch, es_in, d_out, out_group, out_pitch, es_out, omega, phi, scale, stream);
}
extern "C" void dspfft_cztrows_destroy(dspfft_cztrows p)
{
	if (!p) return;
	be_free(p->W); be_free(p->atab);
	delete p;
}
extern "C" int dspfft_transpose_f32(float *d_out, long long out_pitch, const float *d_in, long long in_pitch, int rows, int cols, void *stream)
{
	if (!d_out || !d_in || rows < 1 || cols < 1 || out_pitch < rows || in_pitch < cols) return fail(-1, "bad arguments");
	if (int rc = be_transpose(d_out, out_pitch, d_in, in_pitch, rows, cols, stream)) return fail(-4, "kernel launch failed (transpose): backend code %d", rc);
	return 0;
}

// ---- zoom's animation loop (include/dspfft.h dspfft_zoomanim_*; zoom/zoom.c:320-410) ----
// dspfft_zoomczt_execute's stages (y chirp-z on the transposed coefficients, transpose, x chirp-z), with the plans sized once for the
// largest extents a frame can need (nc = w, h; y lines w 3) and each frame running on its own (cw, ch) <= (w, h).  The coefficients are
// transposed once (set_coeffs); a frame reads the first cw 3 lines and the first ch entries of each.
struct dspfft_zoomanim_s {
	int w, h, type, vw, vh, trc;
	bool coeffs_set;
	float *Ct;                       // the coefficient block transposed: Ct[(u, c)][v], w 3 lines of h
	dspfft_cztrows rows_y, rows_x;
};
namespace {
size_t za_r4(size_t n) { return (n + 3) & ~(size_t)3; }
}  // namespace
extern "C" const char *dspfft_zoomanim_last_error(void) { return g_err; }
extern "C" int dspfft_zoomanim_create(dspfft_zoomanim *out, int w, int h, int type, int vw, int vh)
{
	if (!out) return fail(-1, "null object pointer");
	*out = nullptr;
	if (w < 1 || h < 1 || vw < 1 || vh < 1 || type < 0 || type > 2) return fail(-1, "bad arguments (%dx%d, type %d, view %dx%d)", w, h, type, vw, vh);
	const long long big = vh > h ? vh : h;
	if ((long long)w * 3 * big >= (1ll << 31) || (long long)vw * vh * 3 >= (1ll << 31)) return fail(-2, "frame too large for 31-bit strides");
	dspfft_zoomanim z = new dspfft_zoomanim_s();
	z->w = w; z->h = h; z->type = type; z->vw = vw; z->vh = vh; z->trc = 0; z->coeffs_set = false;
	z->rows_y = z->rows_x = nullptr;
	z->Ct = (float *)be_alloc((size_t)w * 3 * h * sizeof(float));
	if (!z->Ct) { delete z; return fail(-3, "no device memory for the transposed coefficients"); }
	const int ry = dspfft_cztrows_create(&z->rows_y, h, vh, w * 3, 1);
	const int rx = ry ? ry : dspfft_cztrows_create(&z->rows_x, w, vw, vh * 3, 3);
	if (ry || rx) {
		if (z->rows_y) dspfft_cztrows_destroy(z->rows_y);
		be_free(z->Ct);
		delete z;
		return (ry ? ry : rx) == -2 ? -2 : -3;      // (the plan's message stays in g_err)
	}
	*out = z;
	return 0;
}
// Yt (w 3 x vh) | T (vh x w 3) | F (vh x vw x 3: the x stage's interleaved frame when the caller asks for planes)
extern "C" size_t dspfft_zoomanim_work_floats(dspfft_zoomanim z)
{
	if (!z) return 0;
	return za_r4((size_t)z->w * 3 * z->vh) + za_r4((size_t)z->vh * z->w * 3) + za_r4((size_t)z->vh * z->vw * 3);
}
extern "C" int dspfft_zoomanim_set_coeffs(dspfft_zoomanim z, const float *d_coeffs, void *stream)
{
	if (!z || !d_coeffs) return fail(-1, "null object or buffer");
	if (dspfft_transpose_f32(z->Ct, z->h, d_coeffs, (long long)z->w * 3, z->h, z->w * 3, stream)) return -4;
	z->coeffs_set = true;
	return 0;
}
extern "C" int dspfft_zoomanim_execute(dspfft_zoomanim z, double xnum, double xden, double ynum, double yden, double vx, double vy,
                                       int showsamples, int layout, float *d_out, float *d_work, void *stream)
{
	if (!z || !d_out || !d_work) return fail(-1, "null object or buffer");
	if (!z->coeffs_set) return fail(-1, "no coefficients: call dspfft_zoomanim_set_coeffs first");
	if (showsamples < 0 || showsamples > 2 || layout < 0 || layout > 1) return fail(-1, "bad showsamples %d or layout %d", showsamples, layout);
	// a finite scale at or below 1 / len (zero and negative included) is clamped to 1 / len by za_axis, as zoom.c:37-41 does
	if (!(xden > 0) || !(yden > 0) || !std::isfinite(xnum / xden) || !std::isfinite(ynum / yden) || !std::isfinite(vx) || !std::isfinite(vy))
		return fail(-1, "scales must be finite with positive denominators, offsets finite (the caller skips non-finite frames, zoom.c:342-345)");
	if ((showsamples || layout == 1 || z->trc) && !dspfft_zoomanim_finish_launch)
		return fail(-3, "zoom animation overlay / planar store / transfer characteristic: not in this build (the kernel is HIP-only, zoom_anim.hip)");
	const ZaOverlay ov = za_overlay(showsamples, xnum, xden, ynum, yden, vx, vy, z->vw, z->vh);
	const bool finish = ov.mode || layout == 1 || z->trc;
	double wx, px, wy, py;
	const int cw = za_axis(z->type, xnum, xden, z->w, vx, wx, px), ch = za_axis(z->type, ynum, yden, z->h, vy, wy, py);
	if (!cw || !ch) return fail(-2, "centered basis: len * scale must exceed 1");
	const long long cols = (long long)cw * 3;
	float *Yt = d_work, *T = Yt + za_r4((size_t)z->w * 3 * z->vh), *F = T + za_r4((size_t)z->vh * z->w * 3);
	float *X = layout == 1 ? F : d_out;
	// y axis: ch coefficients -> vh samples on the first cw 3 columns; back to rows of cw RGB pixels; x axis into the interleaved frame
	if (dspfft_cztrows_execute_n(z->rows_y, ch, (int)cols, z->Ct, z->h, 0, 1, Yt, z->vh, 0, 1, wy, py, 1.0, stream) ||
	    dspfft_transpose_f32(T, cols, Yt, z->vh, (int)cols, z->vh, stream) ||
	    dspfft_cztrows_execute_n(z->rows_x, cw, z->vh * 3, T, cols, 1, 3, X, (long long)z->vw * 3, 1, 3, wx, px, 1.0 / ((double)z->w * (double)z->h), stream))
		return -4;
	if (finish) {
		char err[256] = "";
		if (dspfft_zoomanim_finish_launch(d_out, X, &ov, layout, z->trc, stream, err, sizeof err)) return fail(-4, "%s", err);
	}
	return 0;
}
extern "C" int dspfft_zoomanim_set_trc(dspfft_zoomanim z, int trc)
{
	if (!z) return fail(-1, "null object");
	if (trc && !trc_built(trc)) return fail(-1, "transfer characteristic %d is not built", trc);
	z->trc = trc;
	return 0;
}
extern "C" void dspfft_zoomanim_destroy(dspfft_zoomanim z)
{
	if (!z) return;
	dspfft_cztrows_destroy(z->rows_y); dspfft_cztrows_destroy(z->rows_x);
	be_free(z->Ct);
	delete z;
}

namespace {
// spec_fused.h is_plain, for the host side: none of the fused scan step's or zoom's extras asked for
bool is_plain_args(const PassArgs &a) { return !a.mask && !a.zflags && !a.accumulate && a.win_hi <= 0 && !a.alt_out && !a.in_mul && !a.in_rev; }
// a planar row pass that can take / produce 8-bit samples itself
// rgb: the caller also takes the 8-bit ends of interleaved RGB lines (spec_inst_row_u8c.hip), whose accesses are whole dwords: it has seen to
// it that every line starts at a multiple of 4 bytes.  The roundtrip and spectrogram calls of motion's planar clips do not ask.
bool pass_has_u8(const dspfft_plan_s *pl, const Pass &P, bool rgb = false)
{
	if (P.type != Pass::ROW || !P.hostloop.empty()) return false;
	// the 8-bit kernels are plain instantiations (spec_kernels.h): a plan with zoom's window / modulation / alternating sign on this axis converts separately
	if (pl->alt_axis == P.axis || (pl->win_axis == P.axis && P.first && pl->zpage)) return false;
	if (P.pa.C == 3 && rgb) return P.has_spec && !P.jit && dspfft_row_u8c_has && dspfft_row_u8c_launch && dspfft_row_u8c_has(P.spec.id);
	if (P.pa.C != 1) return false;
	return (P.has_spec && be_spec_has_u8(P.spec.id)) || (P.jit && P.jit_fn_u8);
}

// motion's -d (dspfft_execute_roundtrip_u8_dither): the bytes come from the dither kernel (motion_dither.hip) instead of the last inverse pass
struct Dither { uint8_t *out8; double sf, norm; };
// the transfer characteristic of one 8-bit end of a roundtrip call (id = 0: none) and its tables on the device
struct U8Trc { int id = 0; const void *tab = nullptr; };
// A plan's first row pass loading ends.in, or its last row pass storing quantise(value * ends.mul) to ends.out, in place in `work`.  trc.id: through
// the listed kernel that has that characteristic's table at its 8-bit end (rt_check has seen to it that the pass has a listed kernel and that
// the launcher is there).
int run_pass_u8(const dspfft_plan_s *pl, const Pass &P, float *work, const U8IO &ends, const U8Trc &trc, void *stream)
{
	const bool last = ends.out != nullptr;
	PassArgs a;
	fill_args(a, P.spa, pl, P, work, work, last ? pl->scale : 1.0, Fuse());
	if (trc.id) {
		U8IOTrc io;
		static_cast<U8IO &>(io) = ends;
		(last ? io.tab_out : io.tab_in) = (const TrcU8Tab *)trc.tab; io.trc_out = last ? trc.id : 0;
		if (int rc = dspfft_row_u8_trc_launch(P.spec.id, &a, &io, P.spec_nwg, stream)) return fail(-4, "kernel launch failed (%s, u8 with a transfer characteristic): backend code %d", P.desc.c_str(), rc);
		return 0;
	}
	if (P.jit && !P.has_spec) {
		U8IO io2 = ends;
		void *args[2] = {&a, &io2};
		if (int rc = be_jit_launch_n(P.jit_fn_u8, args, P.spec_nwg, P.jit_nthr, stream)) return fail(-4, "kernel launch failed (%s, u8): backend code %d", P.desc.c_str(), rc);
		return 0;
	}
	if (P.pa.C == 3) {        // interleaved RGB lines (pass_has_u8 with rgb)
		if (int rc = dspfft_row_u8c_launch(P.spec.id, &a, &ends, P.spec_nwg, stream)) return fail(-4, "kernel launch failed (%s, u8 rgb): backend code %d", P.desc.c_str(), rc);
		return 0;
	}
	if (int rc = be_launch_spec_u8(P.spec.id, a, ends, P.spec_nwg, stream)) return fail(-4, "kernel launch failed (%s, u8): backend code %d", P.desc.c_str(), rc);
	return 0;
}
// the planes of a plan's output layout: its last two axes (rank 1: rows of their own), the first of three and the batch axes index planes
int dither_geom_of(const dspfft_plan_s *p, dspfft_dither_geom &g)
{
	const int r = p->rank;
	if (p->axes[r - 1].os != 1) return fail(-2, "dithered store: the contiguous axis must be the plan's last (planar layout)");
	g.n[0] = r == 3 ? p->n[0] : 1; g.n[1] = r >= 2 ? p->n[r - 2] : 1; g.n[2] = p->n[r - 1];
	g.row_pitch = r >= 2 ? p->axes[r - 2].os : p->n[r - 1];
	g.plane_pitch = r == 3 ? p->axes[0].os : 0;
	int k = 0;
	for (int i = 0; i < 3; i++) { g.nblocks[i] = 1; g.block_step[i] = 0; }
	for (const Dim &b : p->batches) {
		if (b.n == 1) continue;
		if (k == 3) return fail(-2, "dithered store: more than three batch axes");
		g.nblocks[k] = b.n; g.block_step[k] = b.os; k++;
	}
	return 0;
}
int dither_store(const dspfft_plan_s *inv, const float *work, const Dither &dz, const U8Trc &trc, void *stream)
{
	dspfft_dither_geom g;
	if (int rc = dither_geom_of(inv, g)) return rc;
	char err[256] = "";
	if (!dspfft_dither_launch) return fail(-3, "dithered 8-bit store: not in this build");
	if (trc.id ? dspfft_dither_trc_launch(dz.out8, work, &g, dz.sf, dz.norm, trc.id, trc.tab, stream, err, sizeof err)
	           : dspfft_dither_launch(dz.out8, work, &g, dz.sf, dz.norm, stream, err, sizeof err)) return fail(-4, "%s", err);
	return 0;
}

// ---- the fused roundtrip: one call record (RtCall), filled by its entry, checked (rt_check), then run by one strategy (roundtrip_core) ----
// DSPFFT_NO_FUSED_ROUNDTRIP=1: no fused column kernel and no slices.  Read on every call (tests toggle it inside one process).
bool fused_roundtrip_off() { const char *e = getenv("DSPFFT_NO_FUSED_ROUNDTRIP"); return e && *e == '1'; }

// a call's filter parameters, checked, as the kernels take them (fp NULL: no filter, mf all zero); what: the caller's name in the message, or NULL
int motion_filter_of(const dspfft_motion_filter_params *fp, MotionFilter &mf, const char *what = nullptr)
{
	memset((void *)&mf, 0, sizeof mf);
	if (!fp) return 0;
	if (fp->preserve_dc < 0 || fp->preserve_dc > 2 || fp->minbuf_hw[0] < 1 || fp->minbuf_hw[1] < 1 || fp->block_depth < 1) return fail(-1, "%s%sbad filter parameters", what ? what : "", what ? ": " : "");
	motion_filter_from(*fp, mf);
	return 0;
}
bool extents_differ(const dspfft_plan_s *fwd, const dspfft_plan_s *inv) { return fwd->rank != inv->rank || !std::equal(fwd->n, fwd->n + fwd->rank, inv->n); }

// The blocks of a plan pair as motion.c:652-668 sees them: `nblocks` runs of `count` floats (a block's whole embedding, :657), `stride` apart
// in the working buffer.  False when the blocks are no such runs (interleaved batches, blocks lying side by side in a volume).
struct TopnRuns { size_t count, nblocks; long long stride; };
bool topn_runs_of(const dspfft_plan_s *fwd, const dspfft_plan_s *inv, TopnRuns &r)
{
	long long span = 1;
	for (int a = 0; a < fwd->rank; a++) span += (long long)(std::max(fwd->n[a], inv->n[a]) - 1) * fwd->axes[a].os;
	std::vector<Dim> dims;
	for (const Dim &b : fwd->batches) if (b.n > 1) dims.push_back(Dim{b.n, b.os, b.os});
	merge_dims(dims);
	if (dims.size() > 1 || (dims.size() == 1 && dims[0].os < span)) return false;
	r.count = (size_t)span; r.nblocks = dims.empty() ? 1 : (size_t)dims[0].n; r.stride = dims.empty() ? span : dims[0].os;
	return true;
}

// One roundtrip call as its entry fills it: zero but for what the entry has.
// d_in8 / d_out8 non-NULL: 8-bit samples at the two ends (dspfft_execute_roundtrip_u8), d_out is then the float work buffer.
struct RtArgs {
	dspfft_plan fwd, inv;
	const float *d_in; float *d_out; const uint8_t *d_in8; uint8_t *d_out8; double mul8 = 1.0;
	const dspfft_motion_filter_params *fp; unsigned long long *coded; void *stream;
	size_t keep; void *topn_work; size_t topn_work_bytes;       // motion --coeff-limit (rt_limit); keep = 0: none
	double outside_mul;                   // > 0: the call came through a dspfft_execute_roundtrip*_limit entry, which takes a limit on a rescaled block grid
	Dither dither;                        // out8 non-NULL (d_out8 NULL): the inverse ends in d_out as floats and the dither kernel stores the bytes from there;
	                                      // out8 = d_out8 (packed small blocks): the call's one kernel dithers in its tile and stores the bytes itself
	const dspfft_motion_packed *packed;   // non-NULL: dspfft_execute_roundtrip_u8_packed's call, d_in8 / d_out8 hold packed->components bytes per pixel
	bool packed_frames;                   // ... dspfft_execute_roundtrip_u8_packed_frames's: the interleaved full-frame pair, d_out is the float work buffer
	bool packed_rescale;                  // ... dspfft_execute_roundtrip_u8_packed_rescale's: a rescaled block grid, out of place; with keep and outside_mul its _limit
	                                      // twin's, with dither.out8 = d_out8 its _dither twin's (with or without keep)
	bool may_slice = true;               // false: a slice of a clip (roundtrip_sliced)
};
// ... and what rt_check derives from them for the runners (zero before)
struct RtCall : RtArgs {
	const Pass *F, *I;                    // the forward plan's last pass and the inverse plan's first
	bool rescale;                         // the inverse runs over other extents than the forward
	bool block;                           // small blocks on aligned buffers: the fused block pass runs the call
	bool u8_first, u8_last;               // the first forward / last inverse pass is a row pass with an 8-bit kernel of its own
	long long span;                       // extent of the working buffer in elements
	int nf3[3], ni3[3];                   // region geometry of the two ends (rank padded to 3 with unit extents)
	long long sw3[3], si3[3];
	MotionFilter mf;
	TopnRuns runs;                        // keep != 0 and not `block`: the blocks as contiguous runs of the working buffer
	U8Trc trc_in, trc_out;                // dspfft_plan_set_u8_trc of the forward plan (8-bit input) and of the inverse plan (8-bit or dithered output)
	bool grid;                            // a rescaled block grid (rt_grid): block_rescale.hip's kernel runs the call, out of place
	BlockRsTopnArgs rs;                   // its arguments, with the geometry derived for the pair (keep = 0: no coefficient limit; block_rescale_topn.hip's kernel otherwise)
	bool temporal;                        // blocks along time that the plans' own passes cannot run (rt_temporal): temporal_rt.hip's kernel runs the call
	TemporalArgs tp;                      // its arguments but the tables (rt_run_temporal)
	BlockPackedDitherArgs pk;             // packed pixels (rt_packed): block_packed.hip's kernel runs the call, or (c.dither) block_packed_dither.hip's
	BlockRsPackedWideArgs pg;             // packed pixels over a rescaled block grid (rt_packed_grid): block_rescale_packed.hip's kernel runs the call, or, with a
	                                      // coefficient limit (pg.keep) or -d (pg.dither), one of the wide tile's (block_rs_packed_wide_core.h)
	MotionFilterPacked mfp;               // packed pixels over full frames (rt_packed_frames): the filter of the fused column kernel's twin,
	dspfft_motion_filter_params pf_fp;    // ... and of the stand-alone kernel (the call's, with the frame's geometry), over
	int pf_h, pf_w; long long pf_frames;  // ... that many frames of h x w pixels
	bool pf_plain;                        // ... no filter, or one that is position-free and the same for every component: mf runs in the planar fused kernel
	int nwg; size_t lds;                  // the launch of the grid's, the temporal blocks' or the packed pixels' one kernel
};
// the dspfft_coeff_limit of a dspfft_execute_roundtrip*_limit entry into its call: what every such entry refuses of it comes first
int rt_limit(RtCall &c, const dspfft_coeff_limit *cl)
{
	if (!cl) return fail(-1, "coefficient limit: null dspfft_coeff_limit (the entries without one take none)");
	if (!cl->keep) return fail(-1, "coefficient limit: keep must be at least 1 (the entries without a dspfft_coeff_limit take none)");
	if (!std::isfinite(cl->outside_mul) || !(cl->outside_mul > 0)) return fail(-1, "coefficient limit: outside_mul must be finite and > 0 (1 for motion's 3-D blocks)");
	c.keep = cl->keep; c.topn_work = cl->d_work; c.topn_work_bytes = cl->work_bytes; c.outside_mul = cl->outside_mul;
	return 0;
}
// the conversions at the ends of the unfused paths, plain or through the call's transfer characteristic
int rt_u8_in(const RtCall &c, float *dst, uint64_t len)
{
	return c.trc_in.id ? dspfft_u8_trc_flat_launch(dst, c.d_in8, 1.0, len, 0, c.trc_in.id, c.trc_in.tab, c.stream) : be_u8_to_f32(dst, c.d_in8, len, c.stream);
}
int rt_u8_out(const RtCall &c, const float *src, uint64_t len)
{
	return c.trc_out.id ? dspfft_u8_trc_flat_launch(c.d_out8, src, c.mul8, len, 1, c.trc_out.id, c.trc_out.tab, c.stream) : be_f32_to_u8(c.d_out8, src, c.mul8, len, c.stream);
}

// ---- what the checkers of the strategies share ----
int rt_filter(RtCall &c, const char *what = nullptr) { return motion_filter_of(c.fp, c.mf, what); }
// motion --linear: a plan's transfer characteristic acts where the call has an 8-bit end for it
void rt_trc_ends(RtCall &c)
{
	if (c.d_in8 && c.fwd->u8_trc) c.trc_in = U8Trc{c.fwd->u8_trc, c.fwd->u8_tab};
	if ((c.d_out8 || c.dither.out8) && c.inv->u8_trc) c.trc_out = U8Trc{c.inv->u8_trc, c.inv->u8_tab};
}
// ... and its tables, for a fused kernel's arguments (the store has a table only where the kernel stores bytes itself: not ahead of the dither kernel)
template <class Args> void rt_tables(const RtCall &c, Args &a) { a.tab_in = (const TrcU8Tab *)c.trc_in.tab; a.tab_out = c.d_out8 ? (const TrcU8Tab *)c.trc_out.tab : nullptr; a.trc_out = c.trc_out.id; }
// the call's buffers for a fused kernel's arguments: floats or bytes at either end
template <class Args> void rt_buffers(const RtCall &c, Args &a) { a.in = c.d_in8 ? nullptr : c.d_in; a.out = c.d_out8 ? nullptr : c.d_out; a.in8 = c.d_in8; a.out8 = c.d_out8; a.mul8 = c.mul8; }
// the fused block kernels move float4s and packed words of four bytes at the two ends
bool rt_ends_aligned(const RtCall &c)
{
	const uintptr_t pin = c.d_in8 ? (uintptr_t)c.d_in8 : (uintptr_t)c.d_in, pout = c.d_out8 ? (uintptr_t)c.d_out8 : (uintptr_t)c.d_out;
	return !((c.d_in8 ? 3u : 15u) & pin) && !((c.d_out8 ? 3u : 15u) & pout);
}
// the largest group of at most G blocks whose tile leaves room for the tables and the counter in a workgroup's 64 KB of LDS; 0: not even one block does
int rt_lds_group(int G, size_t block_bytes)
{
	while (G > 0 && (size_t)G * block_bytes + sizeof(TrcU8Tab) + 16 > 64 * 1024) G--;
	return G;
}
// The arguments every fused block roundtrip shares: the forward plan's geometry with the inverse plan's output strides spliced in, the
// call's buffers, the two plans' scales, the filter (rt_filter has run) and the counter.
void rt_block_args(const RtCall &c, BlockRtArgs &a)
{
	static_cast<BlockGeom &>(a) = c.fwd->blk;
	const BlockGeom &o = c.inv->blk;
	a.sy_out = o.sy_out; a.sz_out = o.sz_out; a.sxb_out = o.sxb_out;
	for (int d = 0; d < o.nd; d++) a.bos[d] = o.bos[d];
	rt_buffers(c, a);
	block_scales(c.fwd, a.f); block_scales(c.inv, a.i);
	a.filt = c.mf; a.coded = c.coded;
}

constexpr const char *kGrid = "roundtrip with different forward / inverse extents over a grid of blocks";
constexpr const char *kGridBlocks = "every extent of both plans must be 4, 8 or 16 (2-D blocks: 32 too), x contiguous, all strides multiples of 4 (a single block goes with howmany = 1)";
// what a grid asks of its pair beyond different extents (rt_grid, rt_packed_grid); no_blocks: the reason given for a plan without small blocks
int rt_grid_pair(const dspfft_plan_s *fwd, const dspfft_plan_s *inv, const char *what, const char *no_blocks)
{
	if (fwd->rank != inv->rank) return fail(-2, "%s: the plans have different ranks (%d-D blocks against %d-D blocks)", what, fwd->rank, inv->rank);
	if (!fwd->has_block || !inv->has_block) return fail(-2, "%s: %s", what, no_blocks);
	if (fwd->blk_kind != KIND_REDFT10 || inv->blk_kind != KIND_REDFT01) return fail(-2, "%s: the forward plan must be REDFT10 and the inverse REDFT01 on every axis", what);
	const BlockGeom &f = fwd->blk, &i = inv->blk;
	for (int k = 0; k < 3; k++) if (fwd->blk_axis[k] != inv->blk_axis[k]) return fail(-2, "%s: the plans order their axes differently", what);
	if (f.rows_fast != i.rows_fast) return fail(-2, "%s: one plan is a block-major stack and the other the blocks of a volume", what);
	bool same = f.nxb == i.nxb && f.nd == i.nd;
	for (int d = 0; same && d < f.nd; d++) same = f.bn[d] == i.bn[d];
	if (!same || fwd->howmany != inv->howmany) return fail(-2, "%s: the plans count different numbers of blocks", what);
	return 0;
}
// motion -b with -s over a block grid (motion.c:488-499,535-552): both plans cut their volumes into small blocks, `fwd` the input volume
// into blocks of `block`, `inv` the output volume into as many blocks of `scaled`.  0: the pair is none (the call goes on as before: every
// such pair was refused until now); 1: it is one, c.grid and c.rs are set and everything about the call is checked; < 0: it is almost one,
// or the call cannot run.  Nothing is launched here.
int rt_grid(RtCall &c)
{
	const dspfft_plan fwd = c.fwd, inv = c.inv;
	if (!extents_differ(fwd, inv) || fwd->howmany < 2 || inv->howmany < 2) return 0;
	const char *const what = kGrid;
	if (int rc = rt_grid_pair(fwd, inv, what, kGridBlocks)) return rc;
	const BlockGeom &f = fwd->blk, &i = inv->blk;
	if (!dspfft_block_rescale_launch) return fail(-3, "%s: not built into this library (the kernel is HIP-only, block_rescale.hip)", what);
	const int mx = std::max(f.nx, i.nx), my = std::max(f.ny, i.ny), mz = std::max(f.nz, i.nz);
	unsigned int limit = 0;
	if (c.keep && c.keep < (size_t)mx * my * mz) {
		// (the entries without dspfft_coeff_limit have no outside_mul to rank the coefficients outside min(block, scaled) with)
		if (!(c.outside_mul > 0))
			return fail(-2, "%s: a coefficient limit is not implemented here (the reference selects over the whole embedding, motion.c:652-668)", what);
		if (!dspfft_block_rescale_topn_launch) return fail(-3, "%s with a coefficient limit: not built into this library (the kernel is HIP-only, block_rescale_topn.hip)", what);
		limit = (unsigned int)c.keep;
	}
	c.keep = 0;
	if (!rt_ends_aligned(c)) return fail(-2, "%s: float buffers must be 16-byte aligned, 8-bit buffers 4-byte aligned", what);
	if (int rc = rt_filter(c)) return rc;
	rt_trc_ends(c);
	BlockRsTopnArgs &r = c.rs;
	memset((void *)&r, 0, sizeof r);
	rt_block_args(c, r);
	r.ox = i.nx; r.oy = i.ny; r.oz = i.nz;
	// what the reference ranks outside min(block, scaled): the coefficient without the forward plan's scales, times outside_mul (block_rs_core.h)
	r.keep = limit; r.key_mul = limit ? (float)(c.outside_mul / (double)r.f.scale) : 0.f;
	for (int k = 0; k < 3; k++) r.key_mul0[k] = 1.f / r.f.out0[k];
	rt_tables(c, r);
	// blocks per workgroup: build_block's rule on the embedding with tiles of twice the size -- about 8192 samples (32 KB), rows of at most
	// 1 KB.  The pruned phases have min(block, scaled) columns per block, so build_block's 4096 samples leave half the workgroup idle in them
	// (1920x1080x64, 8-bit: 8x8x8 -> 4x4x4 1.17 -> 1.43 TB/s, 16x16x16 -> 8x8x8 0.92 -> 1.29, profiles/r09_motion_block_rescale.txt).  The
	// tables and the counter fit behind such a tile; a forced G gives way until they do.
	int G;
	{
		EnvScope env(fwd->plan_env);
		G = env_int("DSPFFT_BLOCK_G");
	}
	if (G < 1) G = std::min(256 / mx, 8192 / (mx * my * mz));
	G = std::max(1, rt_lds_group(std::max(1, std::min(G, f.nxb)), (size_t)mz * my * mx * sizeof(float)));
	r.tw = mx; r.G = G; r.pitch = G * mx; r.ngroups = (f.nxb + G - 1) / G; r.gdiv = make_div((uint32_t)r.ngroups);
	long long nwg = r.ngroups;
	for (int d = 0; d < r.nd; d++) nwg *= r.bn[d];
	if (nwg > 0x7fffffffLL) return fail(-2, "%s: too many blocks for one launch", what);
	c.nwg = (int)nwg; c.lds = (size_t)mz * my * r.pitch * sizeof(float);
	c.grid = true;
	return 1;
}

// a rescaled block grid: load, forward over `block`, filter, inverse over `scaled`, store -- one launch, from the forward plan's input layout
// into the inverse plan's output layout
int rt_run_grid(const RtCall &c)
{
	if (c.rs.keep) {
		if (int rc = dspfft_block_rescale_topn_launch(&c.rs, c.nwg, c.lds, c.stream)) return fail(-4, "kernel launch failed (rescaled block grid with a coefficient limit): backend code %d", rc);
		return 0;
	}
	if (int rc = dspfft_block_rescale_launch(&c.rs, c.nwg, c.lds, c.stream)) return fail(-4, "kernel launch failed (rescaled block grid): backend code %d", rc);
	return 0;
}

// ---- blocks along time: motion -b 1x1xD, with -s 1x1xD' (motion/README.md:87-89) ----
// A pair is temporal when both plans are f32 and rank 1, REDFT10 / REDFT01, the transformed axis has stride P > 1 on both sides of both
// plans, a unit-stride batch dimension holds exactly the P samples of a frame, and at most one further batch dimension, the blocks, lies
// n P apart (n the plan's own length: fwd over the input clip, inv over the dense output clip), counted alike by both plans.
struct TemporalPair { int D, S, P, nd; };
bool rt_temporal_side(const dspfft_plan_s *pl, int kind, int &n, long long &P, long long &nd)
{
	if (pl->f64 || pl->rank != 1 || pl->kinds[0] != kind) return false;
	const Dim &ax = pl->axes[0];
	n = pl->n[0]; P = ax.is; nd = 1;
	if (n < 2 || ax.is != ax.os || P <= 1) return false;
	bool pixels = false, blocks = false;
	for (const Dim &b : pl->batches) {
		if (b.n == 1) continue;
		if (b.is != b.os) return false;
		if (!pixels && b.is == 1 && b.n == P) pixels = true;
		else if (!blocks && b.is == (long long)n * P) { blocks = true; nd = b.n; }
		else return false;
	}
	return pixels;
}
bool rt_temporal_pair(const dspfft_plan_s *fwd, const dspfft_plan_s *inv, TemporalPair &t)
{
	long long Pf, Pi, nf, ni;
	if (!rt_temporal_side(fwd, DSPFFT_REDFT10, t.D, Pf, nf) || !rt_temporal_side(inv, DSPFFT_REDFT01, t.S, Pi, ni) || Pf != Pi || nf != ni || Pf > 0x7fffffffLL) return false;
	t.P = (int)Pf; t.nd = (int)nf;
	return true;
}
// does the axis of length n factor into the column pass's radices (no prime factor above 13: no Bluestein)?
bool temporal_length_ok(int n)
{
	for (int p : {2, 3, 5, 7, 11, 13}) while (n % p == 0) n /= p;
	return n == 1;
}
// DSPFFT_TEMPORAL_K=16|32|64|128: a narrower tile than the budget allows (measurements; read on every call)
int temporal_forced_k()
{
	const char *e = getenv("DSPFFT_TEMPORAL_K");
	const int k = e ? atoi(e) : 0;
	return (k == 16 || k == 32 || k == 64 || k == 128) ? k : 0;
}

// 0: the pair is not temporal, or the call is one the plans' own passes run as they always did (float, equal extents, no filter or a
// pure quantiser); 1: temporal_rt.hip's kernel runs it -- every 8-bit call, every call with D' != D, every float call whose filter needs
// positions (the stand-alone filter would derive them from a block-major offset) -- c.temporal and c.tp are set and everything about the
// call is checked; < 0: such a call that cannot run.  Nothing is launched and no table is built here.
int rt_temporal(RtCall &c)
{
	TemporalPair t;
	if (!rt_temporal_pair(c.fwd, c.inv, t)) return 0;
	if (int rc = rt_filter(c)) return rc;
	const bool u8 = c.d_in8 || c.d_out8, positional = c.fp && !c.mf.quant_only;
	if (c.dither.out8 || (!u8 && t.D == t.S && !positional)) return 0;      // (roundtrip_dither sends a temporal pair's call here as the plain 8-bit one)
	const char *const what = "roundtrip over blocks along time (motion -b 1x1xD)";
	const int m = std::max(t.D, t.S);
	if (c.keep && c.keep < (size_t)m) return fail(-2, "%s: a coefficient limit is not implemented here", what);
	c.keep = 0;
	if (!temporal_length_ok(t.D) || !temporal_length_ok(t.S))
		return fail(-2, "%s: lengths %d and %d must have no prime factor above 13 (the fused kernel has no Bluestein pass)", what, t.D, t.S);
	int K = temporal_tile_k(m);
	if (!K) return fail(-2, "%s: max(D, D') = %d is too long for the narrowest tile (16 columns in %d KB of LDS: up to %d)", what, m, TEMPORAL_TILE_BYTES / 1024, TEMPORAL_TILE_BYTES / 64);
	if (t.P % 4) return fail(-2, "%s: the samples per frame (the frame pitch), %d, must be a multiple of 4", what, t.P);
	if (!rt_ends_aligned(c)) return fail(-2, "%s: float buffers must be 16-byte aligned, 8-bit buffers 4-byte aligned", what);
	if (const int fk = temporal_forced_k()) K = std::min(K, fk);
	const long long ntiles = ((long long)t.P + K - 1) / K, nwg = ntiles * t.nd;
	if (nwg > 0x7fffffffLL) return fail(-2, "%s: too many workgroups for one launch (%lld tiles of %d columns)", what, nwg, K);
	if (!dspfft_temporal_rt_launch) return fail(-3, "%s: not built into this library (the kernel is HIP-only, temporal_rt.hip)", what);
	rt_trc_ends(c);
	TemporalArgs &a = c.tp;
	memset((void *)&a, 0, sizeof a);
	a.D = t.D; a.S = t.S; a.K = K; a.B = K / 2; a.P = t.P; a.ntiles = (int)ntiles;
	a.blk_in = (long long)t.D * t.P; a.blk_out = (long long)t.S * t.P;
	rt_buffers(c, a);
	a.f_scale = (float)c.fwd->scale; a.f_in0 = (float)c.fwd->in0[0]; a.f_out0 = (float)c.fwd->out0[0];
	a.i_scale = (float)c.inv->scale; a.i_in0 = (float)c.inv->in0[0]; a.i_out0 = (float)c.inv->out0[0];
	a.filt = c.mf; a.coded = c.coded;
	rt_tables(c, a);
	a.divB = make_div((uint32_t)a.B); a.divQ = make_div((uint32_t)(K / 4)); a.div_tiles = make_div((uint32_t)a.ntiles);
	c.nwg = (int)nwg;
	c.temporal = true;
	return 1;
}

// a plan's axis as the column pass sees it: the complex FFT of its full length and the tables T, W, pos (the plan's own pass is a TINY
// pass without tables up to 32 points)
int temporal_tables(dspfft_plan_s *pl)
{
	std::lock_guard<std::mutex> lock(pl->rt_mutex);
	if (pl->temporal) return 0;
	auto P = std::make_unique<Pass>();
	memset(&P->pa, 0, sizeof P->pa);
	std::vector<uint32_t> pos;
	if (!build_fft(pl->n[0], P->pa.fft, pos)) return fail(-2, "roundtrip over blocks along time: length %d does not factor", pl->n[0]);
	if (upload_tables(*P, false, pl->n[0], pl->n[0], pos)) { P->tab.release(); return fail(-3, "table upload failed"); }
	pl->temporal = std::move(P);
	return 0;
}

// blocks along time: load, forward over D, filter by z, inverse over D', store -- one launch from the forward plan's input clip into the
// inverse plan's output clip (the same clip for equal extents in place: a tile reads all its frames before it writes any)
int rt_run_temporal(const RtCall &c)
{
	if (int rc = temporal_tables(c.fwd)) return rc;
	if (int rc = temporal_tables(c.inv)) return rc;
	TemporalArgs a = c.tp;
	const Pass &F = *c.fwd->temporal, &I = *c.inv->temporal;
	a.ff = F.pa.fft; a.fi = I.pa.fft;
	a.Tf = (const cx<float> *)F.tab.T; a.Wf = (const cx<float> *)F.tab.W; a.posf = (const uint32_t *)F.tab.pos;
	a.Ti = (const cx<float> *)I.tab.T; a.Wi = (const cx<float> *)I.tab.W; a.posi = (const uint32_t *)I.tab.pos;
	if (int rc = dspfft_temporal_rt_launch(&a, c.nwg, c.stream)) return fail(-4, "kernel launch failed (blocks along time): backend code %d", rc);
	return 0;
}

// ---- motion on packed 8-bit pixels (rgb24, rgba ...; include/dspfft.h): the planar small-block pair's geometry with every stride and offset
// times `components`, block_packed.hip's kernel.  The entry has refused null plans, buffers and c.packed, f64 plans and a limit of 0; the rest
// of the call is checked here, the library's own lack of the kernel last.  0: c.pk is set; < 0: the call cannot run.  Nothing is launched here.
// Full frames of packed pixels: whether `pl` is the dense in-place interleaved plan of rank 2 over [frames][h][w][C] -- axes {h: stride w C,
// w: stride C}, batch levels {C: stride 1} and, for frames > 1, {frames: stride h w C} -- and how many frames it counts.  -2 with the reason.
int packed_frames_layout(const dspfft_plan_s *pl, int C, const char *what, long long &frames)
{
	const char *const layout = "the plan must be the dense in-place layout [frames][h][w][components]: rank 2, axis strides w * components and components, batch levels {components: stride 1} and {frames: stride h * w * components}";
	if (pl->rank != 2) return fail(-2, "%s: %s", what, layout);
	const int h = pl->n[0], w = pl->n[1];
	const Dim *chan = nullptr;
	for (const Dim &b : pl->batches) if (b.n > 1 && b.is == 1 && b.os == 1 && !chan) chan = &b;
	if (!chan || chan->n != C) return fail(-2, "%s: the plan's unit-stride batch level counts %d, not the %d components of a pixel", what, chan ? chan->n : 0, C);
	const long long frame = (long long)h * w * C;
	frames = 1;
	int levels = 0;
	for (const Dim &b : pl->batches) {
		if (b.n == 1 || &b == chan) continue;
		if (levels++ || b.is != frame || b.os != frame) return fail(-2, "%s: %s", what, layout);
		frames = b.n;
	}
	if (pl->axes[1].is != C || pl->axes[1].os != C || pl->axes[0].is != (long long)w * C || pl->axes[0].os != (long long)w * C) return fail(-2, "%s: %s", what, layout);
	return 0;
}

constexpr const char *kPacked = "roundtrip on packed 8-bit pixels";
constexpr const char *kPackedDither = "dithered roundtrip on packed 8-bit pixels";
int rt_packed(RtCall &c)
{
	const dspfft_plan fwd = c.fwd, inv = c.inv;
	const bool dither = c.dither.out8 != nullptr;           // motion -d: the store's three phases in the tile (block_packed_core.h)
	const char *const what = dither ? kPackedDither : kPacked;
	if (int rc = rt_filter(c, what)) return rc;
	const int C = c.packed->components;
	if (C < 2 || C > PACKED_MAX_COMPS) return fail(-2, "%s: components must be 2, 3 or 4 bytes per pixel, got %d (one component is the planar call)", what, C);
	if (dither && extents_differ(fwd, inv) && fwd->has_block && inv->has_block)
		return fail(-2, "%s: different forward / inverse extents: -d on a packed rescaled grid is not implemented (the tile keeps min(block, scaled) columns and has no room for the scaled planes)", what);
	if (extents_differ(fwd, inv) && fwd->has_block && inv->has_block) return fail(-2, "%s: different forward / inverse extents (a rescaled block grid, motion -s) are not implemented on packed pixels", what);
	if (!block_roundtrip_ok(fwd, inv))
		return fail(-2, "%s needs the plan pair of the fused block pass: matching REDFT10 / REDFT01 small-block plans (every extent 4, 8 or 16, 2-D blocks up to 32; per-frame and single-block plans have no block pass)", what);
	if (!rt_ends_aligned(c)) return fail(-2, "%s: the buffers must be 4-byte aligned", what);
	rt_trc_ends(c);
	BlockPackedDitherArgs &a = c.pk;
	memset((void *)&a, 0, sizeof a);
	rt_block_args(c, a);
	rt_tables(c, a);
	// the plans count pixels; the kernel addresses bytes
	a.sy_in *= C; a.sz_in *= C; a.sxb_in *= C; a.sy_out *= C; a.sz_out *= C; a.sxb_out *= C;
	long long nwg = 1;
	for (int d = 0; d < a.nd; d++) { a.bis[d] *= C; a.bos[d] *= C; nwg *= a.bn[d]; }
	int G = packed_group_of(a.nx, a.ny, a.nz, C, a.nxb);
	if (const char *e = getenv("DSPFFT_PACKED_G")) { if (atoi(e) > 0) G = std::min(atoi(e), a.nxb); }      // experiments (tools/bench_motion_packed.py)
	const size_t block_bytes = (size_t)a.nz * a.ny * C * a.nx * sizeof(float);
	G = rt_lds_group(G, block_bytes);
	// -d: the error table and the dither lanes' error rows lie behind the tile and the tables
	while (dither && G > 0 && (size_t)G * block_bytes + sizeof(TrcU8Tab) + 16 + packed_dither_bytes(a.nx, packed_dither_slots(a.nz, C, G)) > 64 * 1024) G--;
	if (!G && dither)
		return fail(-2, "%s: the %d component tiles of a %dx%dx%d block (%zu bytes), the tables and the dither's error rows do not fit a workgroup's 64 KB of LDS", what, C, a.nx, a.ny, a.nz, block_bytes);
	if (!G) return fail(-2, "%s: the %d component tiles of a %dx%dx%d block (%zu bytes) and the tables do not fit a workgroup's 64 KB of LDS", what, C, a.nx, a.ny, a.nz, block_bytes);
	a.G = G; a.pitch = G * C * a.nx; a.ngroups = (a.nxb + G - 1) / G; a.gdiv = make_div((uint32_t)a.ngroups);
	nwg *= a.ngroups;
	if (nwg > 0x7fffffffLL) return fail(-2, "%s: too many blocks for one launch (more than 2^31 - 1 workgroups)", what);
	a.comps = C;
	if (c.fp) for (int k = 0; k < C; k++) { a.damp[k] = c.packed->damp[k]; a.boost[k] = c.packed->boost[k]; a.grey_add[k] = c.packed->grey_add[k]; }
	// --coeff-limit: at or above the block's count nothing is dropped (motion.c:654-657) and the call is the plain one
	a.keep = c.keep < (size_t)a.nx * a.ny * a.nz ? (unsigned int)c.keep : 0;
	if (dither) { a.sf = c.dither.sf; a.norm = c.dither.norm; a.slots = packed_dither_slots(a.nz, C, G); }
	if (dither && !dspfft_block_packed_dither_launch) return fail(-3, "%s: not built into this library (the kernel is HIP-only, block_packed_dither.hip)", what);
	if (!dspfft_block_packed_launch) return fail(-3, "%s: not built into this library (the kernel is HIP-only, block_packed.hip)", what);
	c.nwg = (int)nwg; c.lds = (size_t)G * block_bytes;
	return 0;
}
int rt_run_packed(const RtCall &c)
{
	if (c.dither.out8) {
		if (int rc = dspfft_block_packed_dither_launch(&c.pk, c.nwg, c.lds, c.stream)) return fail(-4, "kernel launch failed (%s): backend code %d", kPackedDither, rc);
		return 0;
	}
	if (int rc = dspfft_block_packed_launch(&c.pk, c.nwg, c.lds, c.stream)) return fail(-4, "kernel launch failed (%s): backend code %d", kPacked, rc);
	return 0;
}

// ---- motion -b with -s on packed 8-bit pixels (include/dspfft.h): rt_grid's pair -- the PLANAR grid pair over the clip in pixels -- with every stride
// and offset times `components`, block_rescale_packed.hip's kernel.  The entry has refused null plans, buffers and c.packed and f64 plans.
// 0: c.pg is set; < 0: the call cannot run.  Nothing is launched here.
constexpr const char *kPackedGrid = "roundtrip on packed 8-bit pixels over a rescaled grid of blocks";
constexpr const char *kPackedGridLimit = "roundtrip on packed 8-bit pixels over a rescaled grid of blocks with a coefficient limit";
constexpr const char *kPackedGridDither = "dithered roundtrip on packed 8-bit pixels over a rescaled grid of blocks";
// the pixels from a clip's first to one past its last, as the plan's block geometry lays it out (out: the output side)
long long block_clip_span(const BlockGeom &g, bool out)
{
	long long span = (long long)(g.nxb - 1) * (out ? g.sxb_out : g.sxb_in) + (long long)(g.nz - 1) * (out ? g.sz_out : g.sz_in) + (long long)(g.ny - 1) * (out ? g.sy_out : g.sy_in) + g.nx;
	for (int d = 0; d < g.nd; d++) span += (long long)(g.bn[d] - 1) * (out ? g.bos[d] : g.bis[d]);
	return span;
}
int rt_packed_grid(RtCall &c)
{
	const dspfft_plan fwd = c.fwd, inv = c.inv;
	const bool dither = c.dither.out8 != nullptr;           // motion -d: the store's three phases in the wide tile (block_rs_packed_wide_core.h)
	const char *const what = dither ? kPackedGridDither : c.outside_mul > 0 ? kPackedGridLimit : kPackedGrid;          // (outside_mul: the _limit entry's call, whatever its keep)
	if (int rc = rt_filter(c, what)) return rc;
	const int C = c.packed->components;
	if (C < 2 || C > PACKED_MAX_COMPS) return fail(-2, "%s: components must be 2, 3 or 4 bytes per pixel, got %d (one component is the planar call)", what, C);
	if (!extents_differ(fwd, inv)) return fail(-2, "%s: the plans have equal extents: that pair is dspfft_execute_roundtrip_u8_packed's (small blocks) or dspfft_execute_roundtrip_u8_packed_frames's", what);
	if (fwd->howmany < 2 || inv->howmany < 2) return fail(-2, "%s: one block with different extents (howmany = 1) is not implemented on packed pixels", what);
	if (int rc = rt_grid_pair(fwd, inv, what, "every extent of both plans must be 4, 8 or 16 (2-D blocks: 32 too), x contiguous, all strides multiples of 4; full frames of packed pixels are "
	                          "dspfft_execute_roundtrip_u8_packed_frames's, which takes equal extents only (motion -s over full frames is not implemented)")) return rc;
	if (!rt_ends_aligned(c)) return fail(-2, "%s: the buffers must be 4-byte aligned", what);
	const BlockGeom &f = fwd->blk, &i = inv->blk;
	// out of place by nature: the two clips, in bytes
	const uintptr_t in0 = (uintptr_t)c.d_in8, out0 = (uintptr_t)c.d_out8;
	const unsigned long long in_bytes = (unsigned long long)block_clip_span(f, false) * C, out_bytes = (unsigned long long)block_clip_span(i, true) * C;
	if (in0 < out0 + out_bytes && out0 < in0 + in_bytes)
		return fail(-2, "%s: the input clip (%llu bytes) and the output clip (%llu bytes) overlap; the call is out of place (the clips have different extents)", what, in_bytes, out_bytes);
	rt_trc_ends(c);
	BlockRsPackedWideArgs &a = c.pg;
	memset((void *)&a, 0, sizeof a);
	rt_block_args(c, a);
	rt_tables(c, a);
	a.ox = i.nx; a.oy = i.ny; a.oz = i.nz;
	// --coeff-limit: at or above the embedding's count nothing is dropped (motion.c:654-657) and the call is the one without a limit
	const int ex = std::max(f.nx, i.nx);
	const bool limit = c.keep && c.keep < (size_t)ex * std::max(f.ny, i.ny) * std::max(f.nz, i.nz);
	const bool wide = limit || dither;
	// the plans count pixels; the kernel addresses bytes
	a.sy_in *= C; a.sz_in *= C; a.sxb_in *= C; a.sy_out *= C; a.sz_out *= C; a.sxb_out *= C;
	long long nwg = 1;
	for (int d = 0; d < a.nd; d++) { a.bis[d] *= C; a.bos[d] *= C; nwg *= a.bn[d]; }
	// the tile of a component block: the embedding's rows and planes, the active columns (block_rs_packed_core.h)
	// with a limit or -d: the wide tile's columns, the embedding's or `scaled`'s, and rs_packed_group_of's rule on that tile
	const int mx = wide ? rs_packed_wide_tw(f.nx, i.nx, limit) : std::min(f.nx, i.nx), my = std::max(f.ny, i.ny), mz = std::max(f.nz, i.nz);
	int G = rs_packed_group_of(mx, my, mz, f.ny * f.nz, i.ny * i.nz, C, a.nxb);
	bool forced = false;
	if (const char *e = getenv("DSPFFT_PACKED_G")) { if (atoi(e) > 0) { G = std::min(atoi(e), a.nxb); forced = true; } }      // experiments (tools/bench_motion_packed_rescale.py)
	const size_t block_bytes = (size_t)mz * my * C * mx * sizeof(float);
	G = rt_lds_group(G, block_bytes);
	// -d: the error table and, with one lane per plane, the dither lanes' error rows lie behind the tile, the tables and the counter.  The walk leaves
	// most lanes idle, so the rule's group gives way until four workgroups share a CU's 160 KB of LDS (40 KB each) and one's walk hides behind the
	// others' passes: the fastest group of the -d sweeps with a limit and of 8x8x8 -> 4x4x4 without, within 12 % of the fastest elsewhere
	// (profiles/r23_motion_packed_rescale_limit_dither.txt)
	// Which walk (rs_packed_dither_by_rows) is decided on the planes of the largest tile that fits; with oy lanes per plane the group then gives way
	// until its planes fill their rounds of lanes (1x8x8 -> 1x16x16 rgb24: 10.5 ms at ten pixel blocks, 480 lanes in two rounds; 13.8 at twelve, three)
	const bool by_rows = dither && rs_packed_dither_by_rows(i.ny, i.nx, i.nz * C * std::max(1, G));
	const auto dither_lds = [&](int g) { return (size_t)g * block_bytes + sizeof(TrcU8Tab) + 16 + rs_packed_wide_dither_bytes(i.nx, i.nz, C, g, true, by_rows); };
	const auto rounds = [&](int g) { return (i.nz * C * g * i.ny + BLOCK_THREADS - 1) / BLOCK_THREADS; };
	while (dither && G > 0 && dither_lds(G) > 64 * 1024) G--;
	while (dither && !forced && G > 1 && dither_lds(G) > 40 * 1024) G--;
	while (by_rows && !forced && G > 1 && rounds(G) == rounds(G + 1)) G--;
	if (!G && dither)
		return fail(-2, "%s: the %d component tiles of a %dx%dx%d embedding, %d columns each (%zu bytes), the tables and the dither's error rows do not fit a workgroup's 64 KB of LDS", what, C, ex, my, mz, mx, block_bytes);
	if (!G) return fail(-2, "%s: the %d component tiles of a %dx%dx%d embedding (%zu bytes) and the tables do not fit a workgroup's 64 KB of LDS", what, C, ex, my, mz, block_bytes);
	if (limit) {
		// what the reference ranks outside min(block, scaled): the coefficient without the forward plan's scales, times outside_mul (block_rs_core.h)
		bool listed = false;
#define DSP_RS_SEL(K_, MX_) listed = listed || (mx == MX_ && rs_topn_keys(mx * my * mz) == K_);
		DSPFFT_RS_TOPN_SHAPES(DSP_RS_SEL)
#undef DSP_RS_SEL
		if (!listed) return fail(-2, "%s: no selection for a %dx%dx%d embedding", what, mx, my, mz);
		a.keep = (unsigned int)c.keep; a.key_mul = (float)(c.outside_mul / (double)a.f.scale);
		for (int k = 0; k < 3; k++) a.key_mul0[k] = 1.f / a.f.out0[k];
	}
	if (dither) { a.dither = 1; a.sf = c.dither.sf; a.norm = c.dither.norm; a.slots = packed_dither_slots(i.nz, C, G); a.by_rows = by_rows; }
	a.tw = mx; a.G = G; a.pitch = G * C * mx; a.ngroups = (a.nxb + G - 1) / G; a.gdiv = make_div((uint32_t)a.ngroups);
	nwg *= a.ngroups;
	if (nwg > 0x7fffffffLL) return fail(-2, "%s: too many blocks for one launch (more than 2^31 - 1 workgroups)", what);
	a.comps = C;
	if (c.fp) for (int k = 0; k < C; k++) { a.damp[k] = c.packed->damp[k]; a.boost[k] = c.packed->boost[k]; a.grey_add[k] = c.packed->grey_add[k]; }
	if (dither && !dspfft_block_rescale_packed_dither_launch) return fail(-3, "%s: not built into this library (the kernel is HIP-only, block_rescale_packed_dither.hip)", what);
	if (limit && !dither && !dspfft_block_rescale_packed_limit_launch) return fail(-3, "%s: not built into this library (the kernel is HIP-only, block_rescale_packed_limit.hip)", what);
	if (!dspfft_block_rescale_packed_launch) return fail(-3, "%s: not built into this library (the kernel is HIP-only, block_rescale_packed.hip)", what);
	c.nwg = (int)nwg; c.lds = (size_t)G * block_bytes;
	return 0;
}
int rt_run_packed_grid(const RtCall &c)
{
	if (c.pg.dither) {
		if (int rc = dspfft_block_rescale_packed_dither_launch(&c.pg, c.nwg, c.lds, c.stream)) return fail(-4, "kernel launch failed (%s): backend code %d", kPackedGridDither, rc);
		return 0;
	}
	if (c.pg.keep) {
		if (int rc = dspfft_block_rescale_packed_limit_launch(&c.pg, c.nwg, c.lds, c.stream)) return fail(-4, "kernel launch failed (%s): backend code %d", kPackedGridLimit, rc);
		return 0;
	}
	if (int rc = dspfft_block_rescale_packed_launch(&c.pg, c.nwg, c.lds, c.stream)) return fail(-4, "kernel launch failed (%s): backend code %d", kPackedGrid, rc);
	return 0;
}

// ---- motion on packed 8-bit pixels over full frames (the reference's default -b 0x0x1; include/dspfft.h): the interleaved rank-2 pair over
// [F][h][w][C], run by rt_run_passes with the filter of packed pixels in the middle.  The entry has refused null plans, buffers, d_work and
// c.packed and f64 plans.  0: the call is ready for rt_run_passes; < 0: it cannot run.  Nothing is launched here.
constexpr const char *kPackedFrames = "roundtrip on packed 8-bit pixels over full frames";
constexpr const char *kPackedFramesDither = "dithered roundtrip on packed 8-bit pixels over full frames";
// the frames of [F][h][w][C] as dspfft_motion_dither_u8_packed takes them: in pixels
dspfft_dither_geom packed_frames_dither_geom(long long frames, int h, int w)
{
	dspfft_dither_geom g = {};
	g.n[0] = 1; g.n[1] = h; g.n[2] = w; g.row_pitch = w;
	g.nblocks[0] = (int)frames; g.nblocks[1] = g.nblocks[2] = 1; g.block_step[0] = (long long)h * w;
	return g;
}
int rt_packed_frames(RtCall &c)
{
	const dspfft_plan fwd = c.fwd, inv = c.inv;
	const char *const what = c.dither.out8 ? kPackedFramesDither : kPackedFrames;
	if (int rc = rt_filter(c, what)) return rc;
	const int C = c.packed->components;
	if (C < 2 || C > PACKED_MAX_COMPS) return fail(-2, "%s: components must be 2, 3 or 4 bytes per pixel, got %d (one component is the planar call)", what, C);
	if (fwd->has_block || inv->has_block) return fail(-2, "%s: a small-block pair runs as one kernel without a work buffer: dspfft_execute_roundtrip_u8_packed", what);
	if (fwd->rank == 3 || inv->rank == 3) return fail(-2, "%s: one 3-D block of interleaved pixels (motion -b 0x0x0) is not implemented", what);
	if (extents_differ(fwd, inv)) return fail(-2, "%s: different forward / inverse extents (motion -s) are not implemented on packed pixels", what);
	long long frames, iframes;
	if (int rc = packed_frames_layout(fwd, C, what, frames)) return rc;
	if (int rc = packed_frames_layout(inv, C, what, iframes)) return rc;
	const size_t nf = fwd->passes.size(), ni = inv->passes.size();
	bool kinds = frames == iframes && nf == 2 && ni == 2;
	for (int a = 0; a < 2; a++) kinds = kinds && fwd->kinds[a] == DSPFFT_REDFT10 && inv->kinds[a] == DSPFFT_REDFT01;
	if (!kinds || fwd->passes[1].axis != 0 || inv->passes[0].axis != 0)
		return fail(-2, "%s: the pair must be REDFT10 (forward) and REDFT01 (inverse) over the same frames, the inverse running its column pass first (dspfft_plan_guru_r2r_ordered(..., 1))", what);
	const int h = fwd->n[0], w = fwd->n[1];
	const long long frame = (long long)h * w * C;
	if (frame >= (1LL << 32)) return fail(-2, "%s: a frame of 2^32 samples or more", what);
	rt_trc_ends(c);
	if (!dspfft_motion_filter_packed || ((c.trc_in.id || c.trc_out.id) && !dspfft_u8_trc_flat_launch) || (c.dither.out8 && !dspfft_dither_packed_launch))
		return fail(-3, "%s: not built into this library (the kernels are HIP-only, motion_filter_packed.hip)", what);
	if (c.dither.out8) {          // -d: what the dither kernel would refuse after the passes have run is refused here
		if (frames > 0x7fffffffLL) return fail(-2, "%s: too many frames", what);
		const dspfft_dither_geom g = packed_frames_dither_geom(frames, h, w);
		char err[256] = "";
		if (dspfft_dither_packed_launch(nullptr, nullptr, &g, C, c.dither.sf, c.dither.norm, c.trc_out.id, c.trc_out.tab, 1, c.stream, err, sizeof err)) return fail(-2, "%s: %s", what, err);
	}

	c.F = &fwd->passes[1]; c.I = &inv->passes[0];
	c.span = frames * frame;
	c.pf_h = h; c.pf_w = w; c.pf_frames = frames;
	// an 8-bit end rides on the row pass where the pass has the interleaved kernel, every line of bytes starts at a multiple of 4 and the
	// end has no transfer characteristic (those are the flat sweeps' alone)
	const bool lines4 = ((long long)w * C) % 4 == 0;
	c.u8_first = !c.trc_in.id && lines4 && !(3u & (uintptr_t)c.d_in8) && pass_has_u8(fwd, fwd->passes[0], true);
	c.u8_last = !c.trc_out.id && lines4 && !(3u & (uintptr_t)c.d_out8) && pass_has_u8(inv, inv->passes[1], true);
	memset((void *)&c.mfp, 0, sizeof c.mfp);
	c.pf_plain = true;
	if (c.fp) {
		// active = (1, h, w): every component of a frame is a block of its own; the band and the thresholds are the call's
		dspfft_motion_filter_params &q = c.pf_fp;
		q = *c.fp;
		q.active[0] = 1; q.active[1] = h; q.active[2] = w; q.minbuf_hw[0] = h; q.minbuf_hw[1] = w; q.block_depth = 1;
		q.damp = q.boost = 1.f; q.grey_add = 0.f;                 // (what the planar kernel sees when nothing but the quantiser acts)
		motion_filter_from(q, c.mf);
		motion_filter_packed_set(c.mfp, c.mf, h, w, C, c.packed->damp, c.packed->boost, c.packed->grey_add);
		c.pf_plain = c.mfp.quant_only != 0;
	}
	return 0;
}

// every rejection of a roundtrip call; nothing has been launched when it returns
int rt_check(RtCall &c)
{
	const dspfft_plan fwd = c.fwd, inv = c.inv;
	const dspfft_motion_filter_params *fp = c.fp;
	if (c.packed) return c.packed_frames ? rt_packed_frames(c) : c.packed_rescale ? rt_packed_grid(c) : rt_packed(c);      // (their entries take no other strategy, and have seen to plans and buffers)
	if (!fwd || !inv || !(c.d_in || c.d_in8) || !(c.d_out || c.d_out8)) return fail(-1, "null plan or buffer");
	if (fwd->f64 || inv->f64) return fail(-1, "the fused roundtrip takes f32 plans");
	if (int t = rt_temporal(c)) return t < 0 ? t : 0;          // (ahead of rt_grid, which answers every rescaled pair with batches that it is no grid)
	if (int g = rt_grid(c)) return g < 0 ? g : 0;
	if (!c.d_out) return fail(-1, "null plan or buffer");       // (only a rescaled block grid and blocks along time store their bytes without a float work buffer)
	const size_t nf = fwd->passes.size(), ni = inv->passes.size();
	const Pass &F = *(c.F = &fwd->passes[nf - 1]), &I = *(c.I = &inv->passes[0]);
	// (plans whose blocks go through the fused block pass have no pass order to agree on)
	if (fwd->rank != inv->rank || fwd->howmany != inv->howmany || (!extents_differ(fwd, inv) && F.axis != I.axis && !block_roundtrip_ok(fwd, inv)))
		return fail(-1, "the forward plan's last pass and the inverse plan's first pass must run along the same axis (create the inverse with dspfft_plan_many_r2r_ordered(..., 1))");
	// motion's `scaled != block` (motion.c:535-552): the inverse runs over DIFFERENT extents inside the same embedding -- larger:
	// the spectrum is zero-padded (band-limited upscale), smaller: truncated (downscale)
	for (int a = 0; a < fwd->rank; a++) {
		if (fwd->axes[a].os != inv->axes[a].is || inv->axes[a].is != inv->axes[a].os || fwd->kinds[a] != DSPFFT_REDFT10 || inv->kinds[a] != DSPFFT_REDFT01)
			return fail(-1, "roundtrip: the inverse must be REDFT01, in place, on the forward (REDFT10) plan's output layout");
		c.rescale = c.rescale || fwd->n[a] != inv->n[a];
	}
	if (c.rescale && (!fwd->batches.empty() || !inv->batches.empty())) return fail(-2, "roundtrip with different forward / inverse extents takes one block per call (howmany = 1)");
	if (c.rescale)
		for (int a = 0; a < fwd->rank; a++)
			if (fwd->axes[a].is != fwd->axes[a].os) return fail(-2, "roundtrip with different forward / inverse extents needs ONE embedding for input, work and output (motion.c:535-552)");
	if (fwd->batches.size() != inv->batches.size()) return fail(-1, "roundtrip: batch layouts differ");
	for (size_t b = 0; b < fwd->batches.size(); b++)
		if (fwd->batches[b].n != inv->batches[b].n || fwd->batches[b].os != inv->batches[b].is || inv->batches[b].is != inv->batches[b].os) return fail(-1, "roundtrip: batch layouts differ");
	if (int rc = rt_filter(c)) return rc;
	// (the filter addresses the working buffer with 32-bit offsets)
	c.span = 1;
	for (int a = 0; a < fwd->rank; a++) c.span += (long long)(std::max(fwd->n[a], inv->n[a]) - 1) * fwd->axes[a].os;
	for (const Dim &b : fwd->batches) c.span += (long long)(b.n - 1) * b.os;
	if (fp && c.span >= (1ll << 31)) return fail(-2, "filtered roundtrip addresses the buffer with 31-bit offsets: buffer too large");
	for (int k = 0; k < 3; k++) { c.nf3[k] = c.ni3[k] = 1; c.sw3[k] = c.si3[k] = 0; }
	for (int a = 0; a < fwd->rank; a++) {
		const int k = 3 - fwd->rank + a;
		c.nf3[k] = fwd->n[a]; c.ni3[k] = inv->n[a]; c.sw3[k] = fwd->axes[a].os; c.si3[k] = fwd->axes[a].is;
	}
	c.block = !c.rescale && block_roundtrip_ok(fwd, inv) && rt_ends_aligned(c);
	c.u8_first = pass_has_u8(fwd, fwd->passes[0]);
	c.u8_last = pass_has_u8(inv, inv->passes[ni - 1]);
	rt_trc_ends(c);
	if (c.trc_in.id || c.trc_out.id) {
		if (!dspfft_u8_trc_flat_launch || !dspfft_u8_trc_region_launch || !dspfft_dither_trc_launch || !dspfft_block_trc_launch || !dspfft_row_u8_trc_launch)
			return fail(-3, "8-bit roundtrip with a transfer characteristic: not built into this library (the kernels are HIP-only)");
		// the fused ends with tables: the block kernel where the tables fit behind its tile, the listed row kernels (a row kernel compiled at
		// plan time has no such twin: that end is converted by a sweep)
		c.block = c.block && fwd->blk_lds % 16 == 0 && fwd->blk_lds + sizeof(TrcU8Tab) <= 64 * 1024;
		if (c.trc_in.id) c.u8_first = c.u8_first && fwd->passes[0].has_spec && be_spec_has_u8(fwd->passes[0].spec.id);
		if (c.trc_out.id) c.u8_last = c.u8_last && inv->passes[ni - 1].has_spec && be_spec_has_u8(inv->passes[ni - 1].spec.id);
	}
	if (c.keep) {
		// --coeff-limit: at or above the block's embedding count nothing is dropped (motion.c:654-657) and the call is the plain one
		const bool runs = topn_runs_of(fwd, inv, c.runs);
		if (c.block ? c.keep >= (size_t)fwd->blk.nx * fwd->blk.ny * fwd->blk.nz : (runs && c.keep >= c.runs.count)) c.keep = 0;
	}
	if (c.keep) {
		if (!(c.block ? (bool)dspfft_block_topn_launch : (bool)dspfft_topn_blocks_launch && (bool)dspfft_topn_blocks_bytes))
			return fail(-3, "roundtrip with a coefficient limit: not built into this library (the selection kernels are HIP-only, block_topn.hip and motion_ops.hip)");
	}
	if (c.block) return 0;
	// the standalone filter finds a coefficient's position from its offset in a block-major embedding (minbuf_hw, block_depth); the
	// blocks of a volume lying side by side are filtered by the fused block pass only, which knows each block's own coordinates
	if (fp && fwd->has_block && !fwd->blk.rows_fast)
		return fail(-2, "filtered roundtrip over the blocks of a volume needs the fused block pass: matching forward / inverse plans and 16-byte (8-bit: 4-byte) aligned buffers");
	if (c.keep) {
		if (c.runs.count == 0) return fail(-2, "roundtrip with a coefficient limit: every block must be one contiguous run of the working buffer (or go through the fused block pass)");
		if (c.runs.count >= (1ull << 32)) return fail(-2, "roundtrip with a coefficient limit: a block of 2^32 coefficients or more");
		const size_t need = dspfft_topn_blocks_bytes(c.runs.count, c.runs.nblocks);
		if (c.topn_work_bytes < need || (need && !c.topn_work)) return fail(-1, "roundtrip with a coefficient limit: work buffer too small (dspfft_roundtrip_topn_work_bytes)");
	}
	if (c.rescale || !(c.d_in8 || c.d_out8)) return 0;
	// the 8-bit buffers share the plans' element layout; the unfused conversions (rt_run_passes) walk whole spans
	if (nf < 2 || ni < 2) return fail(-2, "8-bit roundtrip needs at least two transformed axes");
	long long ispan = 1, dense = 1;
	for (int a = 0; a < fwd->rank; a++) { ispan += (long long)(fwd->n[a] - 1) * fwd->axes[a].is; dense *= fwd->n[a]; }
	for (const Dim &b : fwd->batches) { ispan += (long long)(b.n - 1) * b.is; dense *= b.n; }
	// the output conversion will be one sweep over the whole span, which must then hold nothing but samples
	if (c.d_out8 && !c.u8_last && dense != c.span) return fail(-2, "8-bit output without a planar specialised row pass needs a dense work layout");
	if (c.d_in8 && !c.u8_first && ispan != c.span) return fail(-2, "8-bit input without a planar specialised row pass needs identical input and work layouts");
	return 0;
}

// small blocks: everything in one pass over the data
int rt_run_block(const RtCall &c)
{
	BlockRtTrcArgs t;          // the arguments of the three kernels: each launcher takes the base it knows
	rt_block_args(c, t);
	t.keep = (unsigned int)c.keep;
	rt_tables(c, t);
	if (c.trc_in.id || c.trc_out.id) {
		if (int rc = dspfft_block_trc_launch(&t, c.fwd->blk_nwg, c.fwd->blk_lds, c.stream)) return fail(-4, "kernel launch failed (fused block roundtrip with a transfer characteristic): backend code %d", rc);
	} else if (c.keep) {
		if (int rc = dspfft_block_topn_launch(&t, c.fwd->blk_nwg, c.fwd->blk_lds, c.stream)) return fail(-4, "kernel launch failed (fused block roundtrip with a coefficient limit): backend code %d", rc);
	} else if (int rc = be_launch_block_roundtrip(t, c.fwd->blk_nwg, c.fwd->blk_lds, c.stream)) return fail(-4, "kernel launch failed (fused block roundtrip): backend code %d", rc);
	return 0;
}

// motion.c:652-668 between the forward passes and the filter, over the blocks as runs; the DCs the filter's preserve_dc = dc restores
// (:734) are those from before the selection (:650)
int rt_topn(const RtCall &c)
{
	if (dspfft_topn_blocks_launch(c.d_out, c.runs.count, c.runs.nblocks, c.runs.stride, c.keep, c.topn_work, c.topn_work_bytes, motion_filter_restores_dc(c.mf), c.stream))
		return fail(-4, "coefficient limit: %s", dspfft_motion_last_error ? dspfft_motion_last_error() : "launch failed");
	return 0;
}

// one block, unfused: zero the working buffer (motion.c:619), load the block region, forward, filter, inverse over the
// scaled region, store it.  In place on a float buffer the caller has zeroed everything outside the block itself.
int rt_run_rescale(const RtCall &c)
{
	const dspfft_plan fwd = c.fwd, inv = c.inv;
	const size_t nf = fwd->passes.size(), ni = inv->passes.size();
	float *const d_out = c.d_out;
	if (c.d_in8) {
		if (be_zero(d_out, (size_t)c.span * sizeof(float), c.stream) ||
		    (c.trc_in.id ? dspfft_u8_trc_region_launch(d_out, c.d_in8, c.nf3, c.sw3, c.si3, 0, 1.0, 1.0, 1.0, c.trc_in.id, c.trc_in.tab, c.stream)
		                 : be_region_u8_to_f32(d_out, c.d_in8, c.nf3, c.sw3, c.si3, c.stream))) return fail(-4, "launch failed");
	} else if (c.d_in != d_out) {
		if (be_zero(d_out, (size_t)c.span * sizeof(float), c.stream)) return fail(-4, "launch failed");
	}
	for (size_t i = 0; i < nf; i++) {
		const Pass &P = fwd->passes[i];
		if (int rc = run_pass<float>(fwd, P, (P.first && !c.d_in8) ? c.d_in : d_out, d_out, i + 1 == nf, c.stream)) return rc;
	}
	if (c.keep) if (int rc = rt_topn(c)) return rc;
	if (c.fp && be_motion_filter(d_out, c.mf, (uint64_t)c.span, c.coded, c.stream)) return fail(-4, "filter launch failed");
	for (size_t i = 0; i < ni; i++)
		if (int rc = run_pass<float>(inv, inv->passes[i], (const float *)d_out, d_out, i + 1 == ni, c.stream)) return rc;
	if (c.d_out8 && (c.trc_out.id ? dspfft_u8_trc_region_launch(c.d_out8, d_out, c.ni3, c.sw3, c.sw3, 1, c.mul8, 1.0, 1.0, c.trc_out.id, c.trc_out.tab, c.stream)
	                              : be_region_f32_to_u8(c.d_out8, d_out, c.mul8, c.ni3, c.sw3, c.sw3, c.stream))) return fail(-4, "launch failed");
	return 0;
}

// fused column launches this process has enqueued so far (listed, packed twin or compiled at plan time): tests tell the fused path from the
// unfused sequence by it, since the results are the same bits
std::atomic<unsigned long long> g_col_roundtrip_launches{0};
// Whether rt_run_passes runs the forward plan's last pass and the inverse plan's first as ONE column kernel, and that kernel's arguments: both
// are COL passes with the same listed kernel (or kernels compiled at plan time for the same type) over the same tiles, plain, without a host
// loop, on 16-byte-aligned buffers, and nothing has to see the whole spectrum in between.  `src` is what the forward plan's last pass reads.
bool rt_col_fused(const RtCall &c, const float *src, PassArgs &af, PassArgs &ai, bool &compiled)
{
	const dspfft_plan fwd = c.fwd, inv = c.inv;
	const Pass &F = *c.F, &I = *c.I;
	const bool listed = F.has_spec && I.has_spec && F.spec.id == I.spec.id;
	compiled = !listed && F.jit && I.jit && F.jit_fn_rt && F.jit_type == I.jit_type;      // kernels compiled at plan time (jit_kernels.h)
	const bool fusable = F.type == Pass::COL && I.type == Pass::COL && (listed || compiled) && F.spec_nwg == I.spec_nwg &&
	                     F.hostloop.empty() && I.hostloop.empty() && (15u & ((uintptr_t)src | (uintptr_t)c.d_out)) == 0 && !fused_roundtrip_off() &&
	                     !c.keep;             // (the selection needs every coefficient of a block before the filter sees one)
	if (!fusable) return false;
	// packed pixels over full frames: the twin with their filter is a listed kernel's only, and addresses the clip with 31-bit offsets -- else
	// the unfused sequence with the frame-local kernel
	if (c.packed && c.fp && c.span >= (1ll << 31)) return false;
	if (c.packed && !c.pf_plain && (compiled || !be_roundtrip_packed_has || !be_roundtrip_packed_has(F.spec.id))) return false;
	fill_args(af, F.spa, fwd, F, src, c.d_out, fwd->scale, Fuse());
	fill_args(ai, I.spa, inv, I, (const float *)c.d_out, c.d_out, inv->passes.size() == 1 ? inv->scale : 1.0, Fuse());
	return is_plain_args(af) && is_plain_args(ai);      // (the fused kernel is the plain instantiation of both passes)
}

// the plans' pass lists, with the forward plan's last and the inverse plan's first pass in one column kernel where there is one
int rt_run_passes(const RtCall &c)
{
	const dspfft_plan fwd = c.fwd, inv = c.inv;
	const size_t nf = fwd->passes.size(), ni = inv->passes.size();
	const Pass &F = *c.F, &I = *c.I;
	float *const d_out = c.d_out;
	void *const stream = c.stream;
	const bool sweep_in = c.d_in8 && !c.u8_first;        // no fused load: one sweep
	if (sweep_in && rt_u8_in(c, d_out, (uint64_t)c.span)) return fail(-4, "launch failed");
	const float *d_in = sweep_in ? d_out : c.d_in;
	for (size_t i = 0; i + 1 < nf; i++) {
		const Pass &P = fwd->passes[i];
		if (i == 0 && c.d_in8 && c.u8_first) {
			if (int rc = run_pass_u8(fwd, P, d_out, U8IO{c.d_in8, nullptr, 1.0}, c.trc_in, stream)) return rc;
			continue;
		}
		if (int rc = run_pass<float>(fwd, P, P.first ? d_in : d_out, d_out, false, stream)) return rc;
	}
	const float *src = nf == 1 ? d_in : d_out;
	PassArgs af, ai;
	bool compiled;
	if (rt_col_fused(c, src, af, ai, compiled)) {
		g_col_roundtrip_launches.fetch_add(1, std::memory_order_relaxed);
		if (compiled) {
			// parameters: (PassArgs af, PassArgs ai, FilterOp filt, unsigned long long *coded); FilterOp is the MotionFilter, nothing else
			void *args[4] = {&af, &ai, (void *)&c.mf, (void *)&c.coded};
			if (int rc = be_jit_launch_n(F.jit_fn_rt, args, F.spec_nwg, F.jit_nthr, stream)) return fail(-4, "kernel launch failed (fused roundtrip, compiled at plan time): backend code %d", rc);
		} else if (c.packed && !c.pf_plain) {
			if (int rc = be_launch_roundtrip_packed(F.spec.id, af, ai, c.mfp, c.coded, F.spec_nwg, stream)) return fail(-4, "kernel launch failed (fused roundtrip, packed pixels): backend code %d", rc);
		} else if (int rc = be_launch_roundtrip(F.spec.id, af, ai, c.mf, c.coded, F.spec_nwg, stream)) return fail(-4, "kernel launch failed (fused roundtrip): backend code %d", rc);
	} else {
		if (int rc = run_pass<float>(fwd, F, src, d_out, true, stream)) return rc;
		if (c.keep) if (int rc = rt_topn(c)) return rc;
		if (c.fp && (c.packed ? dspfft_motion_filter_packed(d_out, c.pf_h, c.pf_w, c.packed->components, (size_t)c.pf_frames, &c.pf_fp, c.packed, c.coded, stream)
		                      : be_motion_filter(d_out, c.mf, (uint64_t)c.span, c.coded, stream))) return fail(-4, "filter launch failed");
		if (int rc = run_pass<float>(inv, I, (const float *)d_out, d_out, ni == 1, stream)) return rc;
	}
	for (size_t i = 1; i < ni; i++) {
		const Pass &P = inv->passes[i];
		if (i + 1 == ni && c.d_out8 && c.u8_last) {
			if (int rc = run_pass_u8(inv, P, d_out, U8IO{nullptr, c.d_out8, c.mul8}, c.trc_out, stream)) return rc;
			continue;
		}
		if (int rc = run_pass<float>(inv, P, (const float *)d_out, d_out, i + 1 == ni, stream)) return rc;
	}
	if (c.d_out8 && !c.u8_last && rt_u8_out(c, d_out, (uint64_t)c.span)) return fail(-4, "launch failed");    // no fused store: one sweep
	return 0;
}

// ---- a clip of frames in slices (motion's per-frame blocks, motion/motion.c:591,613-615: the frames are independent) ----
// The three launches of the 8-bit roundtrip move the clip's float intermediate through HBM four times (2.1 GB for config 5's luma plane).  Walked
// in slices of S frames -- 8-bit rows -> fused column roundtrip -> 8-bit rows per slice, every slice through the SAME S frames of the work
// buffer -- the intermediate stays in the 256 MB Infinity Cache and only the 8-bit ends touch HBM.  What that buys is bounded by the kernels,
// which are issue- and latency-bound rather than HBM-bound (profiles/r06_motion_slices.txt): the column kernel gains 5-10 % on a resident slice
// with the narrow K = 8 tile (four workgroups per CU; on the HBM-resident clip K = 16's 64-byte segments win), the row kernels lose a few per
// cent to the launch tails of eleven launches instead of one.  Slices alternate between the caller's stream and one of the library's own with a
// work area each, so that one slice's launch tails fill with the other's kernels.
// Which plans: 2-D f32 per-frame plans with ONE batch level whose column pass has a narrow-tile entry (spec_list.h) and whose clip is larger
// than two slices.  DSPFFT_RT_SLICE=frames forces a slice size (0: never), DSPFFT_RT_STREAMS=1 keeps every slice on the caller's stream.
constexpr size_t kSliceBytes = 100u << 20;        // per work area (two areas in flight: 200 MB of the cache's 256)
constexpr int kSliceTileK = 8;

// the two slice switches, read once per process
struct SliceSwitches { int forced, nstreams; };
const SliceSwitches &slice_switches()
{
	static const SliceSwitches s = []() {
		const char *f = getenv("DSPFFT_RT_SLICE"), *n = getenv("DSPFFT_RT_STREAMS");
		return SliceSwitches{f ? atoi(f) : -1, std::min(2, std::max(1, n ? atoi(n) : 2))};
	}();
	return s;
}

int slice_frames(const dspfft_plan_s *fwd, const dspfft_plan_s *inv, const dspfft_motion_filter_params *fp)
{
	const int forced = slice_switches().forced, nstreams = slice_switches().nstreams;
	if (forced == 0 || fwd->rank != 2 || fwd->batches.size() != 1 || inv->batches.size() != 1 || fwd->passes.size() != 2 || inv->passes.size() != 2) return 0;
	if (fwd->col_kpref || inv->col_kpref) return 0;                     // (a slice plan itself)
	const Pass &F = fwd->passes[1], &I = inv->passes[0];
	if (F.type != Pass::COL || I.type != Pass::COL || !F.has_spec || !I.has_spec || F.jit || I.jit) return 0;
	SpecInfo narrow;
	if (!be_find_spec(1, F.pa.N, F.pa.ninner, &narrow, kSliceTileK) || narrow.P != kSliceTileK || narrow.P == F.spec.P) return 0;
	const Dim &b = fwd->batches[0];
	const long long frame = b.os;                                       // floats between frames of the work layout
	if (frame <= 0 || inv->batches[0].is != b.os || inv->batches[0].os != b.os) return 0;
	long long S = forced > 0 ? forced : (long long)(kSliceBytes * (nstreams > 1 ? 1 : 2) / ((size_t)frame * sizeof(float)));
	if (forced <= 0 && b.n < 4 * S) S = (b.n + 3) / 4;                  // a short clip (a rank's share of a clip split over eight GPUs): four slices,
	const int bd = fp ? fp->block_depth : 1;                            // the filter finds a frame's place in its block from its offset in the work area
	if (bd > 1) S -= S % bd;
	if (S < 1 || (forced <= 0 && S < 8)) return 0;                      // of at least eight frames each (32 frames: 0.369 -> 0.356 ms; fewer: launch tails take over)
	return (int)std::min<long long>(S, b.n);
}

// a slice plan is planned as its parent was: under the parent's snapshot of the planner's switches and its planning effort
struct EffortScope {
	const int prev = t_plan_effort;
	explicit EffortScope(int effort) { t_plan_effort = effort; }
	~EffortScope() { t_plan_effort = prev; }
};
dspfft_plan_s *slice_plan(const dspfft_plan_s *of, int frames)
{
	dspfft_plan_s *pl = new dspfft_plan_s();
	pl->rank = of->rank; pl->scale = of->scale; pl->f64 = of->f64;
	for (int a = 0; a < of->rank; a++) { pl->n[a] = of->n[a]; pl->kinds[a] = of->kinds[a]; pl->in0[a] = of->in0[a]; pl->out0[a] = of->out0[a]; pl->axes[a] = of->axes[a]; }
	if (frames > 1) pl->batches.push_back(Dim{frames, of->batches[0].is, of->batches[0].os});
	pl->col_kpref = kSliceTileK;
	EnvScope env(of->plan_env);
	EffortScope effort(of->plan_effort);
	dspfft_plan out = nullptr;
	return plan_finish(pl, &out, of->first_axis_first) ? nullptr : out;
}
// the parent's scales may have been set since its slice plans were made (dspfft_plan_set_scale / _set_axis_scale0), and its transfer
// characteristic (dspfft_plan_set_u8_trc); the tables stay the parent's
void follow_parent(std::initializer_list<dspfft_plan_s *> slices, const dspfft_plan_s *of)
{
	for (dspfft_plan_s *q : slices) {
		if (!q) continue;
		q->scale = of->scale; q->u8_trc = of->u8_trc; q->u8_tab = of->u8_tab;
		for (int a = 0; a < 2; a++) { q->in0[a] = of->in0[a]; q->out0[a] = of->out0[a]; }
	}
}
// From the fork on, the join of the library's stream: on every way out of roundtrip_sliced the caller's stream waits for what the side stream
// was given, so that nothing of this call writes the caller's buffers once the caller's stream is through.  (Sets no error text: the first
// error's stays.)
struct SideJoin {
	dspfft_plan_s::RtSlices *r;               // NULL: nothing to join (one stream, or joined already)
	void *stream;
	int join()
	{
		dspfft_plan_s::RtSlices *q = std::exchange(r, nullptr);
		if (!q || !(be_event_record(q->ev_join, q->side) || be_stream_wait_event(stream, q->ev_join))) return 0;
		be_stream_synchronize(q->side);
		return -1;
	}
	~SideJoin() { join(); }
};

// returns 1 when the clip was run in slices, 0 when this call does not qualify (the caller runs it whole), < 0 on error
int roundtrip_core(RtCall &c);
int roundtrip_sliced(const RtCall &c)
{
	const dspfft_plan fwd = c.fwd, inv = c.inv;
	const int S = slice_frames(fwd, inv, c.fp);
	if (!S) return 0;
	std::lock_guard<std::mutex> lock(fwd->rt_mutex);
	const int total = fwd->batches[0].n, rem = total % S;
	dspfft_plan_s::RtSlices *r = nullptr;
	for (const auto &q : fwd->rt_slices) if (q->inv_of == inv && q->frames == S) r = q.get();
	if (!r) {
		auto n = std::make_unique<dspfft_plan_s::RtSlices>();
		const bool two = slice_switches().nstreams > 1;
		n->inv_of = inv; n->frames = S;
		n->fwd = slice_plan(fwd, S); n->inv = slice_plan(inv, S);
		if (rem) { n->fwd_rem = slice_plan(fwd, rem); n->inv_rem = slice_plan(inv, rem); }
		if (two) { n->side = be_stream_create(); n->ev_fork = be_order_event_create(); n->ev_join = be_order_event_create(); }
		bool ok = n->fwd && n->inv && (!rem || (n->fwd_rem && n->inv_rem)) && (!two || (n->side && n->ev_fork && n->ev_join));
		// slices without the 8-bit row kernels would take another, slower path than the clip does: the clip then runs whole
		for (dspfft_plan_s *q : {n->fwd, n->fwd_rem}) ok = ok && (!q || pass_has_u8(q, q->passes.front()));
		for (dspfft_plan_s *q : {n->inv, n->inv_rem}) ok = ok && (!q || pass_has_u8(q, q->passes.back()));
		if (!ok) return 0;
		r = n.get();
		fwd->rt_slices.push_back(std::move(n));
	}
	follow_parent({r->fwd, r->fwd_rem}, fwd);
	follow_parent({r->inv, r->inv_rem}, inv);
	const long long fin = fwd->batches[0].is, fwk = fwd->batches[0].os, fout = inv->batches[0].os;
	const bool two = r->side != nullptr;
	if (two && (be_event_record(r->ev_fork, c.stream) || be_stream_wait_event(r->side, r->ev_fork))) return fail(-4, "stream fork failed");
	SideJoin side = {two ? r : nullptr, c.stream};
	int k = 0;
	for (int f0 = 0; f0 < total; f0 += S, k++) {
		const bool last = total - f0 < S, odd = two && (k & 1);
		// the clip's call on the slice's plans, frames, work area and stream: each slice's planes (whole frames) are stored or dithered on the
		// slice's stream before its work area is reused
		RtCall s = {};
		static_cast<RtArgs &>(s) = c;
		s.fwd = last ? r->fwd_rem : r->fwd; s.inv = last ? r->inv_rem : r->inv; s.stream = odd ? r->side : c.stream; s.may_slice = false;
		s.d_out = c.d_out + (odd ? (long long)S * fwk : 0); s.d_in8 = c.d_in8 + (long long)f0 * fin;
		if (c.d_out8) s.d_out8 = c.d_out8 + (long long)f0 * fout;
		if (c.dither.out8) s.dither.out8 = c.dither.out8 + (long long)f0 * fout;
		if (int rc = roundtrip_core(s)) return rc;
	}
	return side.join() ? fail(-4, "stream join failed") : 1;
}

// a call as its entry filled it: checked, then run by the one strategy that takes it
int roundtrip_core(RtCall &c)
{
	if (int rc = rt_check(c)) return rc;
	int rc = 0;
	if (c.packed) rc = c.packed_frames ? rt_run_passes(c) : c.packed_rescale ? rt_run_packed_grid(c) : rt_run_packed(c);
	else if (c.grid) rc = rt_run_grid(c);
	else if (c.temporal) rc = rt_run_temporal(c);
	else if (c.block) rc = rt_run_block(c);
	else if (c.rescale) rc = rt_run_rescale(c);
	else {
		if (c.may_slice && !c.keep && c.d_in8 && (c.d_out8 || c.dither.out8) && c.u8_first && c.u8_last && c.F->axis == c.I->axis && (15u & (uintptr_t)c.d_out) == 0 &&
		    !fused_roundtrip_off())
			rc = roundtrip_sliced(c);
		if (rc) return rc < 0 ? rc : 0;          // in slices: every slice has stored or dithered its own frames
		rc = rt_run_passes(c);
	}
	if (rc || !c.dither.out8 || c.d_out8) return rc;          // (d_out8 beside dither.out8: packed small blocks, dithered in the kernel's tile)
	if (c.packed) {
		const dspfft_dither_geom g = packed_frames_dither_geom(c.pf_frames, c.pf_h, c.pf_w);
		char err[256] = "";
		if (dspfft_dither_packed_launch(c.dither.out8, c.d_out, &g, c.packed->components, c.dither.sf, c.dither.norm, c.trc_out.id, c.trc_out.tab, 0, c.stream, err, sizeof err))
			return fail(-4, "%s", err);
		return 0;
	}
	return dither_store(c.inv, c.d_out, c.dither, c.trc_out, c.stream);
}

// dspfft_execute_roundtrip_u8_dither and its twin with a coefficient limit: the call with the bytes' buffer and the two factors in c.dither
int roundtrip_dither(RtCall &c)
{
	const Dither dz = c.dither;
	if (!c.fwd || !c.inv || !c.d_in8 || !dz.out8) return fail(-1, "null plan or buffer");
	// blocks along time: a 1 x 1 plane has no neighbour to diffuse into (the conditions of motion.c:781-785 are all false), so the bytes
	// are the plain 8-bit call's with out_mul = scalefactor normalization^2 -- and that call needs no work buffer
	TemporalPair tp;
	const bool temporal = rt_temporal_pair(c.fwd, c.inv, tp);
	if (!temporal) {
		if (!c.d_out) return fail(-1, "null plan or buffer");
		if (c.fwd->f64 || c.inv->f64) return fail(-1, "the dithered roundtrip takes f32 plans");
		if (!dspfft_dither_launch) return fail(-3, "dithered 8-bit store: not in this build (the dither kernel is HIP-only, motion_dither.hip)");
	}
	if (!(dz.sf > 0) || !(dz.norm > 0)) return fail(-1, "dither: scalefactor and normalization must be > 0");
	if (temporal) {
		c.d_out8 = dz.out8; c.mul8 = dz.sf * dz.norm * dz.norm; c.dither = Dither{};
		return roundtrip_core(c);
	}
	dspfft_dither_geom g;
	if (int rc = dither_geom_of(c.inv, g)) return rc;
	return roundtrip_core(c);
}
}  // namespace

extern "C" int dspfft_execute_roundtrip(dspfft_plan fwd, dspfft_plan inv, const float *d_in, float *d_out,
                                        const dspfft_motion_filter_params *fp, unsigned long long *d_coeffs_coded, void *stream)
{
	if (!d_in) return fail(-1, "null plan or buffer");
	RtCall c = {};
	c.fwd = fwd; c.inv = inv; c.d_in = d_in; c.d_out = d_out; c.fp = fp; c.coded = d_coeffs_coded; c.stream = stream;
	return roundtrip_core(c);
}

extern "C" int dspfft_execute_roundtrip_u8(dspfft_plan fwd, dspfft_plan inv, const uint8_t *d_in, uint8_t *d_out, float *d_work, double out_mul,
                                           const dspfft_motion_filter_params *fp, unsigned long long *d_coeffs_coded, void *stream)
{
	if (!d_in || !d_out) return fail(-1, "null plan or buffer");         // (d_work: rt_check; a rescaled block grid needs none)
	RtCall c = {};
	c.fwd = fwd; c.inv = inv; c.d_in8 = d_in; c.d_out8 = d_out; c.d_out = d_work; c.mul8 = out_mul; c.fp = fp; c.coded = d_coeffs_coded; c.stream = stream;
	return roundtrip_core(c);
}

// ---- motion --spectrogram / --ispectrogram: the halves of the roundtrip, one plan each (include/dspfft.h) ----
namespace {
struct SpecCall {
	dspfft_plan pl; bool inverse, u8;
	const void *d_in; void *d_out; float *d_work;
	const dspfft_motion_spec_params *sp; const dspfft_motion_filter_params *fp; double out_mul;
	unsigned long long *coded; void *stream;
};

// small blocks: one kernel (block_spec.hip).  Float pixels: the end that is not next to the encode / decode is a factor of the transform
// and rides on the plan's global scale (sample * 255 on the way in, motion.c:623; value * out_mul / 255 on the way out, :759-774).
int spec_block(const SpecCall &c, const MotionFilter &mf)
{
	const dspfft_plan pl = c.pl;
	const char *const what = c.inverse ? "ispectrogram" : "spectrogram";
	if (!dspfft_block_spec_launch) return fail(-3, "%s over small blocks: not built into this library (the kernels are HIP-only, block_spec.hip)", what);
	const unsigned mask = c.u8 ? 3u : 15u;
	if ((mask & (uintptr_t)c.d_in) || (mask & (uintptr_t)c.d_out)) return fail(-2, "%s over small blocks: float buffers must be 16-byte aligned, 8-bit buffers 4-byte aligned", what);
	BlockSpecArgs a;
	memset((void *)&a, 0, sizeof a);
	static_cast<BlockGeom &>(a) = pl->blk;
	if (c.u8) { a.in8 = (const uint8_t *)c.d_in; a.out8 = (uint8_t *)c.d_out; } else { a.in = (const float *)c.d_in; a.out = (float *)c.d_out; }
	block_scales(pl, a.s);
	if (!c.u8) a.s.scale = c.inverse ? (float)(pl->scale * c.out_mul / 255.0) : (float)(pl->scale * 255.0);
	a.filt = mf; a.coded = c.coded; a.mul8 = c.out_mul;
	a.sp = MotionSpec{c.sp->mode, c.sp->scalefactor, c.sp->normalization, c.sp->c};
	if (int rc = dspfft_block_spec_launch(&a, c.inverse, pl->blk_nwg, pl->blk_lds, c.stream)) return fail(-4, "kernel launch failed (%s over small blocks): backend code %d", what, rc);
	return 0;
}

// every other plan: the plan's passes in d_work and motion_ops.hip's kernel over all blocks of the batch at the encoded end
int spec_passes(const SpecCall &c)
{
	const dspfft_plan pl = c.pl;
	const char *const what = c.inverse ? "ispectrogram" : "spectrogram";
	if (!c.d_work) return fail(-1, "%s: this plan needs the float work buffer", what);
	if (!dspfft_spec_blocks_launch) return fail(-3, "%s: not built into this library (the kernels are HIP-only, motion_ops.hip)", what);
	const int r = pl->rank;
	const char *const layout = "the plan must be in place on one planar layout: input strides = output strides, x contiguous, the planes of a block one pitch apart, at most one batch level";
	for (int a = 0; a < r; a++) if (pl->axes[a].is != pl->axes[a].os) return fail(-2, "%s: %s", what, layout);
	if (pl->axes[r - 1].os != 1) return fail(-2, "%s: %s", what, layout);
	int n3[3] = {1, 1, pl->n[r - 1]}, hw[2] = {1, pl->n[r - 1]};
	if (r >= 2) { n3[1] = pl->n[r - 2]; hw[0] = n3[1]; hw[1] = (int)pl->axes[r - 2].os; if (pl->axes[r - 2].os < n3[2] || pl->axes[r - 2].os > 0x7fffffffLL) return fail(-2, "%s: %s", what, layout); }
	if (r == 3) {
		n3[0] = pl->n[0];
		const long long plane = pl->axes[0].os;
		if (plane % hw[1] || plane / hw[1] < n3[1] || plane / hw[1] > 0x7fffffffLL) return fail(-2, "%s: %s", what, layout);
		hw[0] = (int)(plane / hw[1]);
	}
	for (const Dim &b : pl->batches) if (b.n > 1 && b.is != b.os) return fail(-2, "%s: %s", what, layout);
	TopnRuns runs;          // the blocks of the batch: one run each
	if (!topn_runs_of(pl, pl, runs)) return fail(-2, "%s: %s", what, layout);
	const long long span = (long long)runs.count + (long long)(runs.nblocks - 1) * runs.stride;
	long long dense = (long long)runs.nblocks;
	for (int a = 0; a < r; a++) dense *= pl->n[a];
	const size_t np = pl->passes.size();
	// the 8-bit end on the transform's side: the first (last) pass where it is a planar row pass with an 8-bit kernel, else one sweep
	const bool fused8 = c.u8 && np >= 2 && pass_has_u8(pl, pl->passes[c.inverse ? np - 1 : 0]);
	if (c.u8 && c.inverse && !fused8 && dense != span) return fail(-2, "%s: 8-bit output without a planar specialised row pass needs a dense layout", what);
	float *const w = c.d_work;
	const dspfft_motion_spec_params plain_in = {DSPFFT_MOTION_NONE, 1.0, 1.0, 0.0}, plain_out = {DSPFFT_MOTION_NONE, c.out_mul, 1.0, 0.0};
	auto blocks = [&](int inverse, void *pix, const dspfft_motion_spec_params *sp, const dspfft_motion_filter_params *fp, unsigned long long *coded) {
		if (dspfft_spec_blocks_launch(inverse, c.u8, pix, w, n3, hw, runs.nblocks, runs.stride, sp, fp, coded, c.stream))
			return fail(-4, "%s: %s", what, dspfft_motion_last_error ? dspfft_motion_last_error() : "launch failed");
		return 0;
	};
	if (!c.inverse) {
		if (c.u8 && !fused8 && be_u8_to_f32(w, (const uint8_t *)c.d_in, (uint64_t)span, c.stream)) return fail(-4, "launch failed");
		if (!c.u8) if (int rc = blocks(1, (void *)c.d_in, &plain_in, nullptr, nullptr)) return rc;            // sample * 255 (motion.c:623)
		for (size_t i = 0; i < np; i++) {
			const Pass &P = pl->passes[i];
			if (i == 0 && fused8) {
				if (int rc = run_pass_u8(pl, P, w, U8IO{(const uint8_t *)c.d_in, nullptr, 1.0}, U8Trc(), c.stream)) return rc;
			} else if (int rc = run_pass<float>(pl, P, (const float *)w, w, i + 1 == np, c.stream)) return rc;
		}
		return blocks(0, c.d_out, c.sp, c.fp, c.coded);
	}
	if (int rc = blocks(1, (void *)c.d_in, c.sp, c.fp, c.coded)) return rc;
	for (size_t i = 0; i < np; i++) {
		const Pass &P = pl->passes[i];
		if (i + 1 == np && fused8) {
			if (int rc = run_pass_u8(pl, P, w, U8IO{nullptr, (uint8_t *)c.d_out, c.out_mul}, U8Trc(), c.stream)) return rc;
		} else if (int rc = run_pass<float>(pl, P, (const float *)w, w, i + 1 == np, c.stream)) return rc;
	}
	if (c.u8) return !fused8 && be_f32_to_u8((uint8_t *)c.d_out, w, c.out_mul, (uint64_t)span, c.stream) ? fail(-4, "launch failed") : 0;
	return blocks(0, c.d_out, &plain_out, nullptr, nullptr);                                                  // value * out_mul / 255 (:759-774)
}

// every rejection of this function, of spec_block and of spec_passes comes before the first launch (what the kernels' own launchers refuse
// beyond that -- a block of 2^32 samples -- surfaces from spec_passes after its earlier sweeps have written d_work)
int spec_core(const SpecCall &c)
{
	const dspfft_plan pl = c.pl;
	const char *const what = c.inverse ? "ispectrogram" : "spectrogram";
	if (!pl || !c.d_in || !c.d_out || !c.sp) return fail(-1, "null plan or buffer");
	if (pl->f64) return fail(-2, "%s: f64 plans are not implemented", what);
	if (pl->u8_trc) return fail(-2, "%s: a plan with a transfer characteristic (dspfft_plan_set_u8_trc) is not implemented", what);
	const int m = c.sp->mode;
	if (c.inverse && m == DSPFFT_MOTION_ABS) return fail(-2, "ispectrogram: the reference has no abs type (motion.c:627-630): shift, flat or copy");
	if (m != DSPFFT_MOTION_ABS && m != DSPFFT_MOTION_SHIFT && m != DSPFFT_MOTION_FLAT && m != DSPFFT_MOTION_COPY) return fail(-1, "%s: mode must be %sshift, flat or copy", what, c.inverse ? "" : "abs, ");
	for (int a = 0; a < pl->rank; a++)
		if (pl->kinds[a] != (c.inverse ? DSPFFT_REDFT01 : DSPFFT_REDFT10)) return fail(-1, "%s: the plan must be %s on every axis", what, c.inverse ? "REDFT01" : "REDFT10");
	MotionFilter mf;
	if (int rc = motion_filter_of(c.fp, mf)) return rc;
	if (pl->has_block) return spec_block(c, mf);
	return spec_passes(c);
}
}  // namespace

extern "C" int dspfft_execute_spectrogram_u8(dspfft_plan fwd, const uint8_t *d_in, uint8_t *d_out, float *d_work, const dspfft_motion_spec_params *sp,
                                             const dspfft_motion_filter_params *fp, unsigned long long *d_coeffs_coded, void *stream)
{
	return spec_core(SpecCall{fwd, false, true, d_in, d_out, d_work, sp, fp, 1.0, d_coeffs_coded, stream});
}
extern "C" int dspfft_execute_spectrogram_f32(dspfft_plan fwd, const float *d_in, float *d_out, float *d_work, const dspfft_motion_spec_params *sp,
                                              const dspfft_motion_filter_params *fp, unsigned long long *d_coeffs_coded, void *stream)
{
	return spec_core(SpecCall{fwd, false, false, d_in, d_out, d_work, sp, fp, 1.0, d_coeffs_coded, stream});
}
extern "C" int dspfft_execute_ispectrogram_u8(dspfft_plan inv, const uint8_t *d_in, uint8_t *d_out, float *d_work, const dspfft_motion_spec_params *sp,
                                              const dspfft_motion_filter_params *fp, double out_mul, unsigned long long *d_coeffs_coded, void *stream)
{
	return spec_core(SpecCall{inv, true, true, d_in, d_out, d_work, sp, fp, out_mul, d_coeffs_coded, stream});
}
extern "C" int dspfft_execute_ispectrogram_f32(dspfft_plan inv, const float *d_in, float *d_out, float *d_work, const dspfft_motion_spec_params *sp,
                                               const dspfft_motion_filter_params *fp, double out_mul, unsigned long long *d_coeffs_coded, void *stream)
{
	return spec_core(SpecCall{inv, true, false, d_in, d_out, d_work, sp, fp, out_mul, d_coeffs_coded, stream});
}

// ---- motion --spectrogram / --ispectrogram on packed 8-bit pixels (rgb24, rgba ...; include/dspfft.h): two plan families, told apart by the plan ----
namespace {
struct SpecPackedCall {
	dspfft_plan pl; bool inverse;
	const uint8_t *d_in; uint8_t *d_out; float *d_work;
	const dspfft_motion_spec_params *sp; const dspfft_motion_filter_params *fp; const dspfft_motion_packed *packed; double out_mul;
	unsigned long long *coded; void *stream;
};
const char *spec_packed_name(const SpecPackedCall &c) { return c.inverse ? "ispectrogram on packed 8-bit pixels" : "spectrogram on packed 8-bit pixels"; }

// (A) small blocks: the PLANAR small-block plan's geometry with every stride and offset times `components`, block_spec_packed.hip's kernel
int spec_packed_block(const SpecPackedCall &c, const MotionFilter &mf)
{
	const dspfft_plan pl = c.pl;
	const char *const what = spec_packed_name(c);
	const int C = c.packed->components;
	if ((3u & (uintptr_t)c.d_in) || (3u & (uintptr_t)c.d_out)) return fail(-2, "%s over small blocks: the buffers must be 4-byte aligned", what);
	BlockSpecPackedArgs a;
	memset((void *)&a, 0, sizeof a);
	static_cast<BlockGeom &>(a) = pl->blk;
	a.in8 = c.d_in; a.out8 = c.d_out; a.mul8 = c.out_mul;
	block_scales(pl, c.inverse ? a.i : a.f);
	a.filt = mf; a.coded = c.coded;
	a.sp = MotionSpec{c.sp->mode, c.sp->scalefactor, c.sp->normalization, c.sp->c};
	// the plan counts pixels; the kernel addresses bytes
	a.sy_in *= C; a.sz_in *= C; a.sxb_in *= C; a.sy_out *= C; a.sz_out *= C; a.sxb_out *= C;
	long long nwg = 1;
	for (int d = 0; d < a.nd; d++) { a.bis[d] *= C; a.bos[d] *= C; nwg *= a.bn[d]; }
	const size_t block_bytes = (size_t)a.nz * a.ny * C * a.nx * sizeof(float);
	const int G = rt_lds_group(packed_group_of(a.nx, a.ny, a.nz, C, a.nxb), block_bytes);
	if (!G) return fail(-2, "%s: the %d component tiles of a %dx%dx%d block (%zu bytes) do not fit a workgroup's 64 KB of LDS", what, C, a.nx, a.ny, a.nz, block_bytes);
	a.G = G; a.pitch = G * C * a.nx; a.ngroups = (a.nxb + G - 1) / G; a.gdiv = make_div((uint32_t)a.ngroups);
	nwg *= a.ngroups;
	if (nwg > 0x7fffffffLL) return fail(-2, "%s: too many blocks for one launch (more than 2^31 - 1 workgroups)", what);
	a.comps = C;
	if (c.fp) for (int k = 0; k < C; k++) { a.damp[k] = c.packed->damp[k]; a.boost[k] = c.packed->boost[k]; a.grey_add[k] = c.packed->grey_add[k]; }
	if (!dspfft_block_spec_packed_launch) return fail(-3, "%s over small blocks: not built into this library (the kernels are HIP-only, block_spec_packed.hip)", what);
	if (int rc = dspfft_block_spec_packed_launch(&a, c.inverse, (int)nwg, (size_t)G * block_bytes, c.stream)) return fail(-4, "kernel launch failed (%s over small blocks): backend code %d", what, rc);
	return 0;
}

// (B) full frames (motion's default -b 0x0x1): the caller's in-place, dense, interleaved plan of rank 2 over [F][H][W][C] -- its passes in
// d_work, the first (last) with the interleaved 8-bit row end where it has one, and motion_spec_packed.hip's kernel once over all frames at
// the encoded end.  The call is the composition dspfft_u8_to_f32 -> dspfft_execute -> dspfft_motion_spec_blocks_u8_packed, and its mirror.
int spec_packed_frames(const SpecPackedCall &c)
{
	const dspfft_plan pl = c.pl;
	const char *const what = spec_packed_name(c);
	const int C = c.packed->components;
	if (pl->rank == 3) return fail(-2, "%s: one 3-D block of interleaved pixels (motion -b 0x0x0) is not implemented", what);
	if (!c.d_work) return fail(-1, "%s: this plan needs the float work buffer", what);
	long long frames;
	if (int rc = packed_frames_layout(pl, C, what, frames)) return rc;
	const int h = pl->n[0], w = pl->n[1];
	const long long frame = (long long)h * w * C;
	if (frame >= (1LL << 32)) return fail(-2, "%s: a frame of 2^32 samples or more", what);
	if (!dspfft_spec_frames_packed_launch) return fail(-3, "%s: not built into this library (the kernels are HIP-only, motion_spec_packed.hip)", what);

	float *const wk = c.d_work;
	const uint64_t len = (uint64_t)frames * (uint64_t)frame;
	const std::vector<Pass> &passes = pick_passes(pl, wk, wk);
	const size_t np = passes.size();
	// the 8-bit end on the transform's side rides on the row pass where the plain passes run, the pass has the interleaved kernel and every
	// line of bytes starts at a multiple of 4
	const uint8_t *const bytes = c.inverse ? c.d_out : c.d_in;
	const bool dwords = !(3u & (uintptr_t)bytes) && ((long long)w * C) % 4 == 0;
	const bool fused8 = &passes == &pl->passes && np >= 2 && dwords && pass_has_u8(pl, passes[c.inverse ? np - 1 : 0], true);
	auto frames_kernel = [&](uint8_t *pix) {
		if (dspfft_spec_frames_packed_launch(c.inverse, pix, wk, h, w, C, (size_t)frames, c.sp, c.fp, c.packed, c.coded, c.stream))
			return fail(-4, "%s: %s", what, dspfft_motion_last_error ? dspfft_motion_last_error() : "launch failed");
		return 0;
	};
	if (!c.inverse) {
		if (fused8) {
			if (int rc = run_pass_u8(pl, passes[0], wk, U8IO{c.d_in, nullptr, 1.0}, U8Trc(), c.stream)) return rc;
			for (size_t i = 1; i < np; i++) if (int rc = run_pass<float>(pl, passes[i], (const float *)wk, wk, i + 1 == np, c.stream)) return rc;
		} else {
			if (be_u8_to_f32(wk, c.d_in, len, c.stream)) return fail(-4, "launch failed");
			if (int rc = execute_t<float>(pl, wk, wk, c.stream)) return rc;
		}
		return frames_kernel(c.d_out);
	}
	if (int rc = frames_kernel((uint8_t *)c.d_in)) return rc;
	if (fused8) {
		for (size_t i = 0; i + 1 < np; i++) if (int rc = run_pass<float>(pl, passes[i], (const float *)wk, wk, false, c.stream)) return rc;
		return run_pass_u8(pl, passes[np - 1], wk, U8IO{nullptr, c.d_out, c.out_mul}, U8Trc(), c.stream);
	}
	if (int rc = execute_t<float>(pl, wk, wk, c.stream)) return rc;
	return be_f32_to_u8(c.d_out, wk, c.out_mul, len, c.stream) ? fail(-4, "launch failed") : 0;
}

// every rejection of this function and of the two above comes before the first launch
int spec_packed_core(const SpecPackedCall &c)
{
	const dspfft_plan pl = c.pl;
	const char *const what = spec_packed_name(c);
	if (!pl || !c.d_in || !c.d_out || !c.sp) return fail(-1, "%s: null plan, buffer or parameters", what);
	if (!c.packed) return fail(-1, "%s: null dspfft_motion_packed", what);
	const int C = c.packed->components;
	if (C < 2 || C > PACKED_MAX_COMPS) return fail(-2, "%s: components must be 2, 3 or 4 bytes per pixel, got %d (one component is the planar call)", what, C);
	if (pl->f64) return fail(-2, "%s: f64 plans are not implemented", what);
	if (pl->u8_trc) return fail(-2, "%s: a plan with a transfer characteristic (dspfft_plan_set_u8_trc) is not implemented", what);
	const int m = c.sp->mode;
	if (c.inverse && m == DSPFFT_MOTION_ABS) return fail(-2, "%s: the reference has no abs type (motion.c:627-630): shift, flat or copy", what);
	if (m != DSPFFT_MOTION_ABS && m != DSPFFT_MOTION_SHIFT && m != DSPFFT_MOTION_FLAT && m != DSPFFT_MOTION_COPY) return fail(-1, "%s: mode must be %sshift, flat or copy", what, c.inverse ? "" : "abs, ");
	for (int a = 0; a < pl->rank; a++)
		if (pl->kinds[a] != (c.inverse ? DSPFFT_REDFT01 : DSPFFT_REDFT10)) return fail(-1, "%s: the plan must be %s on every axis", what, c.inverse ? "REDFT01" : "REDFT10");
	MotionFilter mf;
	if (int rc = motion_filter_of(c.fp, mf, what)) return rc;
	if (pl->has_block) return spec_packed_block(c, mf);
	return spec_packed_frames(c);
}
}  // namespace

extern "C" int dspfft_execute_spectrogram_u8_packed(dspfft_plan fwd, const uint8_t *d_in, uint8_t *d_out, float *d_work, const dspfft_motion_spec_params *sp,
                                                    const dspfft_motion_filter_params *fp, const dspfft_motion_packed *packed, unsigned long long *d_coeffs_coded, void *stream)
{
	return spec_packed_core(SpecPackedCall{fwd, false, d_in, d_out, d_work, sp, fp, packed, 1.0, d_coeffs_coded, stream});
}
extern "C" int dspfft_execute_ispectrogram_u8_packed(dspfft_plan inv, const uint8_t *d_in, uint8_t *d_out, float *d_work, const dspfft_motion_spec_params *sp,
                                                     const dspfft_motion_filter_params *fp, const dspfft_motion_packed *packed, double out_mul, unsigned long long *d_coeffs_coded,
                                                     void *stream)
{
	return spec_packed_core(SpecPackedCall{inv, true, d_in, d_out, d_work, sp, fp, packed, out_mul, d_coeffs_coded, stream});
}

// ---- spec / ispec on 8-bit images (include/dspfft.h; the sweeps are spec_image.hip's, their arithmetic spec_image_core.h's) ----
namespace {
struct SpecImageCall {
	dspfft_plan pl; bool inverse;
	const uint8_t *d_in; uint8_t *d_out; const uint8_t *map_in; uint8_t *map_out;
	float *d_work; double *d_dc; const double *dc; int restore_dc;
	const dspfft_spec_image_params *sp; void *stream;
};

// every rejection comes before the first launch
int spec_image_core(const SpecImageCall &c)
{
	const dspfft_plan pl = c.pl;
	const char *const what = c.inverse ? "ispec_u8" : "spec_u8";
	if (!pl || !c.d_in || !c.d_out || !c.sp) return fail(-1, "%s: null plan, buffer or parameters", what);
	const dspfft_spec_image_params &sp = *c.sp;
	if (sp.rangetype < 0 || sp.rangetype > 2 || sp.scaletype < 0 || sp.scaletype > 1 || sp.signtype < 0 || sp.signtype > 3 || !(sp.gain == sp.gain) || sp.gain == 0.0)
		return fail(-1, "%s: bad range / scale / sign code or gain", what);
	if (pl->f64) return fail(-2, "%s: f64 plans are not implemented", what);
	const int kind = c.inverse ? DSPFFT_REDFT01 : DSPFFT_REDFT10;
	if (pl->rank != 2) return fail(-2, "%s: the plan must be of rank 2 (an image), not %d", what, pl->rank);
	if (pl->kinds[0] != kind || pl->kinds[1] != kind) return fail(-2, "%s: the plan must be %s on both axes", what, c.inverse ? "REDFT01" : "REDFT10");
	const int h = pl->n[0], w = pl->n[1], d = pl->howmany;
	std::vector<Dim> dims;
	for (const Dim &b : pl->batches) if (b.n > 1) dims.push_back(b);
	merge_dims(dims);
	const bool chan_ok = dims.empty() ? d == 1 : dims.size() == 1 && dims[0].n == d && dims[0].is == 1 && dims[0].os == 1;
	if (!chan_ok || pl->axes[1].is != d || pl->axes[1].os != d || pl->axes[0].is != (long long)w * d || pl->axes[0].os != (long long)w * d)
		return fail(-2, "%s: the plan must be a dense in-place layout of h x w pixels with the channels interleaved (howmany = channels, stride = channels, dist = 1)", what);
	if (pl->first_axis_first != c.inverse || pl->passes.size() != 2)
		return fail(-2, "%s: the plan's pass order must be %s", what, c.inverse ? "first axis first (dspfft_plan_many_r2r_ordered(..., 1)): the row pass ends it" : "the default: the row pass begins it");
	if (d > SPEC_IMAGE_MAX_CH) return fail(-2, "%s: %d channels (the decode handles up to %d)", what, d, (int)SPEC_IMAGE_MAX_CH);
	if ((c.map_in || c.map_out) && sp.signtype != SPEC_SIGN_ABS) return fail(-2, "%s: a sign map goes with sign type abs only (ispec.c:91)", what);
	if (c.inverse && (sp.rangetype != SPEC_RANGE_ONE || c.restore_dc) && !c.dc)
		return fail(-2, "ispec_u8: the DC values from the spectrogram header are required for range dc/dcs and for DC restoration");
	if (!c.d_work) return fail(-2, "%s: the float work buffer is required", what);
	if (!dspfft_spec_image_encode_launch || !dspfft_spec_image_decode_launch) return fail(-3, "%s: not built into this library (the kernels are HIP-only, spec_image.hip)", what);

	float *const wk = c.d_work;
	const uint64_t len = (uint64_t)h * w * d;
	const std::vector<Pass> &passes = pick_passes(pl, wk, wk);
	// the 8-bit end on the transform's side rides on the row pass where the plain passes run (execute_t's choice: no block kernel, no split
	// pair), the pass has the kernel and every line of bytes starts at a multiple of 4
	const uint8_t *const bytes = c.inverse ? c.d_out : c.d_in;
	const bool dwords = !(3u & (uintptr_t)bytes) && ((long long)w * d) % 4 == 0;
	const bool blocky = pl->has_block && !(15u & (uintptr_t)wk);
	const bool fused8 = !blocky && &passes == &pl->passes && dwords && pass_has_u8(pl, passes[c.inverse ? 1 : 0], true);
	if (!c.inverse) {
		if (fused8) {
			if (int rc = run_pass_u8(pl, passes[0], wk, U8IO{c.d_in, nullptr, 1.0}, U8Trc(), c.stream)) return rc;
			if (int rc = run_pass<float>(pl, passes[1], (const float *)wk, wk, true, c.stream)) return rc;
		} else {
			if (be_u8_to_f32(wk, c.d_in, len, c.stream)) return fail(-4, "launch failed");
			if (int rc = execute_t<float>(pl, wk, wk, c.stream)) return rc;
		}
		SpecImageEnc e;
		e.f = wk; e.out = c.d_out; e.signmap = c.map_out; e.dc = c.d_dc; e.len = len; e.d = d;
		e.gain = sp.gain; e.rangetype = sp.rangetype; e.scaletype = sp.scaletype; e.signtype = sp.signtype;
		if (dspfft_spec_image_encode_launch(&e, c.stream)) return fail(-4, "spec_u8: launch failed");
		return 0;
	}
	SpecImageDec e;
	e.in = c.d_in; e.signmap = c.map_in; e.f = wk; e.len = len; e.d = d;
	e.gain = sp.gain; e.scaletype = sp.scaletype; e.signtype = sp.signtype; e.restore_dc = c.restore_dc ? 1 : 0;
	for (int z = 0; z < SPEC_IMAGE_MAX_CH; z++) { e.mx[z] = 0; e.dc[z] = c.dc && z < d ? c.dc[z] : 0; }
	spec_image_decode_max(e.mx, e.dc, d, sp.gain, sp.rangetype, sp.scaletype);
	if (dspfft_spec_image_decode_launch(&e, c.stream)) return fail(-4, "ispec_u8: launch failed");
	if (fused8) {
		if (int rc = run_pass<float>(pl, passes[0], (const float *)wk, wk, false, c.stream)) return rc;
		return run_pass_u8(pl, passes[1], wk, U8IO{nullptr, c.d_out, 255.0}, U8Trc(), c.stream);
	}
	if (int rc = execute_t<float>(pl, wk, wk, c.stream)) return rc;
	return be_f32_to_u8(c.d_out, wk, 255.0, len, c.stream) ? fail(-4, "launch failed") : 0;
}
}  // namespace

extern "C" int dspfft_execute_spec_u8(dspfft_plan fwd, const uint8_t *d_in, uint8_t *d_out, uint8_t *d_signmap, float *d_work, double *d_dc,
                                      const dspfft_spec_image_params *sp, void *stream)
{
	return spec_image_core(SpecImageCall{fwd, false, d_in, d_out, nullptr, d_signmap, d_work, d_dc, nullptr, 0, sp, stream});
}
extern "C" int dspfft_execute_ispec_u8(dspfft_plan inv, const uint8_t *d_in, const uint8_t *d_signmap, uint8_t *d_out, float *d_work, const double *dc,
                                       int restore_dc, const dspfft_spec_image_params *sp, void *stream)
{
	return spec_image_core(SpecImageCall{inv, true, d_in, d_out, d_signmap, nullptr, d_work, nullptr, dc, restore_dc, sp, stream});
}

extern "C" size_t dspfft_roundtrip_topn_work_bytes(dspfft_plan fwd, dspfft_plan inv)
{
	TopnRuns r;
	if (!fwd || !inv || fwd->f64 || inv->f64 || fwd->rank != inv->rank || block_roundtrip_ok(fwd, inv) || !dspfft_topn_blocks_bytes || !topn_runs_of(fwd, inv, r)) return 0;
	return dspfft_topn_blocks_bytes(r.count, r.nblocks);
}

extern "C" int dspfft_execute_roundtrip_topn(dspfft_plan fwd, dspfft_plan inv, const float *d_in, float *d_out, const dspfft_motion_filter_params *fp, size_t keep,
                                             void *d_topn_work, size_t work_bytes, unsigned long long *d_coeffs_coded, void *stream)
{
	if (!d_in) return fail(-1, "null plan or buffer");
	RtCall c = {};
	c.fwd = fwd; c.inv = inv; c.d_in = d_in; c.d_out = d_out; c.fp = fp; c.coded = d_coeffs_coded; c.stream = stream;
	c.keep = keep; c.topn_work = d_topn_work; c.topn_work_bytes = work_bytes;
	return roundtrip_core(c);
}

extern "C" int dspfft_execute_roundtrip_u8_topn(dspfft_plan fwd, dspfft_plan inv, const uint8_t *d_in, uint8_t *d_out, float *d_work, double out_mul,
                                                const dspfft_motion_filter_params *fp, size_t keep, void *d_topn_work, size_t work_bytes,
                                                unsigned long long *d_coeffs_coded, void *stream)
{
	if (!d_in || !d_out) return fail(-1, "null plan or buffer");
	RtCall c = {};
	c.fwd = fwd; c.inv = inv; c.d_in8 = d_in; c.d_out8 = d_out; c.d_out = d_work; c.mul8 = out_mul; c.fp = fp; c.coded = d_coeffs_coded; c.stream = stream;
	c.keep = keep; c.topn_work = d_topn_work; c.topn_work_bytes = work_bytes;
	return roundtrip_core(c);
}

extern "C" int dspfft_execute_roundtrip_u8_dither(dspfft_plan fwd, dspfft_plan inv, const uint8_t *d_in, uint8_t *d_out, float *d_work,
                                                  double scalefactor, double normalization, const dspfft_motion_filter_params *fp,
                                                  unsigned long long *d_coeffs_coded, void *stream)
{
	RtCall c = {};
	c.fwd = fwd; c.inv = inv; c.d_in8 = d_in; c.d_out = d_work; c.dither = Dither{d_out, scalefactor, normalization}; c.fp = fp; c.coded = d_coeffs_coded; c.stream = stream;
	return roundtrip_dither(c);
}

extern "C" int dspfft_execute_roundtrip_limit(dspfft_plan fwd, dspfft_plan inv, const float *d_in, float *d_out, const dspfft_motion_filter_params *fp,
                                              const dspfft_coeff_limit *cl, unsigned long long *d_coeffs_coded, void *stream)
{
	RtCall c = {};
	if (int rc = rt_limit(c, cl)) return rc;
	if (!d_in) return fail(-1, "null plan or buffer");
	c.fwd = fwd; c.inv = inv; c.d_in = d_in; c.d_out = d_out; c.fp = fp; c.coded = d_coeffs_coded; c.stream = stream;
	return roundtrip_core(c);
}

extern "C" int dspfft_execute_roundtrip_u8_limit(dspfft_plan fwd, dspfft_plan inv, const uint8_t *d_in, uint8_t *d_out, float *d_work, double out_mul,
                                                 const dspfft_motion_filter_params *fp, const dspfft_coeff_limit *cl, unsigned long long *d_coeffs_coded, void *stream)
{
	RtCall c = {};
	if (int rc = rt_limit(c, cl)) return rc;
	if (!d_in || !d_out) return fail(-1, "null plan or buffer");
	c.fwd = fwd; c.inv = inv; c.d_in8 = d_in; c.d_out8 = d_out; c.d_out = d_work; c.mul8 = out_mul; c.fp = fp; c.coded = d_coeffs_coded; c.stream = stream;
	return roundtrip_core(c);
}

extern "C" int dspfft_execute_roundtrip_u8_dither_limit(dspfft_plan fwd, dspfft_plan inv, const uint8_t *d_in, uint8_t *d_out, float *d_work,
                                                        double scalefactor, double normalization, const dspfft_motion_filter_params *fp,
                                                        const dspfft_coeff_limit *cl, unsigned long long *d_coeffs_coded, void *stream)
{
	RtCall c = {};
	if (int rc = rt_limit(c, cl)) return rc;
	c.fwd = fwd; c.inv = inv; c.d_in8 = d_in; c.d_out = d_work; c.dither = Dither{d_out, scalefactor, normalization}; c.fp = fp; c.coded = d_coeffs_coded; c.stream = stream;
	return roundtrip_dither(c);
}

// motion on packed 8-bit pixels (rt_packed).  cl NULL: no coefficient limit.
extern "C" int dspfft_execute_roundtrip_u8_packed(dspfft_plan fwd, dspfft_plan inv, const uint8_t *d_in, uint8_t *d_out, double out_mul,
                                                  const dspfft_motion_filter_params *fp, const dspfft_motion_packed *packed, const dspfft_coeff_limit *cl,
                                                  unsigned long long *d_coeffs_coded, void *stream)
{
	if (!fwd || !inv || !d_in || !d_out) return fail(-1, "%s: null plan or buffer", kPacked);
	if (!packed) return fail(-1, "%s: null dspfft_motion_packed", kPacked);
	if (fwd->f64 || inv->f64) return fail(-1, "%s takes f32 plans", kPacked);
	if (cl && !cl->keep) return fail(-1, "%s: coefficient limit: keep must be at least 1 (pass NULL for no limit)", kPacked);
	RtCall c = {};
	c.fwd = fwd; c.inv = inv; c.d_in8 = d_in; c.d_out8 = d_out; c.mul8 = out_mul; c.fp = fp; c.packed = packed; c.coded = d_coeffs_coded; c.stream = stream;
	if (cl) c.keep = cl->keep;
	return roundtrip_core(c);
}

// ... over full frames (rt_packed_frames): the interleaved pair, through rt_run_passes in d_work
extern "C" int dspfft_execute_roundtrip_u8_packed_frames(dspfft_plan fwd, dspfft_plan inv, const uint8_t *d_in, uint8_t *d_out, float *d_work, double out_mul,
                                                         const dspfft_motion_filter_params *fp, const dspfft_motion_packed *packed,
                                                         unsigned long long *d_coeffs_coded, void *stream)
{
	if (!fwd || !inv || !d_in || !d_out) return fail(-1, "%s: null plan or buffer", kPackedFrames);
	if (!d_work) return fail(-1, "%s: null float work buffer (frames * h * w * components floats)", kPackedFrames);
	if (!packed) return fail(-1, "%s: null dspfft_motion_packed", kPackedFrames);
	if (fwd->f64 || inv->f64) return fail(-1, "%s takes f32 plans", kPackedFrames);
	RtCall c = {};
	c.fwd = fwd; c.inv = inv; c.d_in8 = d_in; c.d_out8 = d_out; c.d_out = d_work; c.mul8 = out_mul; c.fp = fp; c.packed = packed; c.packed_frames = true;
	c.coded = d_coeffs_coded; c.stream = stream;
	return roundtrip_core(c);
}

// the two packed calls above with motion's -d.  Small blocks: block_packed_dither.hip's kernel stores the bytes itself, so the call carries both
// d_out8 and c.dither; full frames: the inverse ends as floats in d_work and dspfft_motion_dither_u8_packed's kernels store the bytes
extern "C" int dspfft_execute_roundtrip_u8_packed_dither(dspfft_plan fwd, dspfft_plan inv, const uint8_t *d_in, uint8_t *d_out, double scalefactor, double normalization,
                                                         const dspfft_motion_filter_params *fp, const dspfft_motion_packed *packed, const dspfft_coeff_limit *cl,
                                                         unsigned long long *d_coeffs_coded, void *stream)
{
	if (!fwd || !inv || !d_in || !d_out) return fail(-1, "%s: null plan or buffer", kPackedDither);
	if (!packed) return fail(-1, "%s: null dspfft_motion_packed", kPackedDither);
	if (fwd->f64 || inv->f64) return fail(-1, "%s takes f32 plans", kPackedDither);
	if (cl && !cl->keep) return fail(-1, "%s: coefficient limit: keep must be at least 1 (pass NULL for no limit)", kPackedDither);
	if (!(scalefactor > 0) || !(normalization > 0) || !std::isfinite(scalefactor) || !std::isfinite(normalization))
		return fail(-1, "%s: scalefactor and normalization must be finite and > 0", kPackedDither);
	RtCall c = {};
	c.fwd = fwd; c.inv = inv; c.d_in8 = d_in; c.d_out8 = d_out; c.dither = Dither{d_out, scalefactor, normalization}; c.mul8 = scalefactor * normalization * normalization;
	c.fp = fp; c.packed = packed; c.coded = d_coeffs_coded; c.stream = stream;
	if (cl) c.keep = cl->keep;
	return roundtrip_core(c);
}

extern "C" int dspfft_execute_roundtrip_u8_packed_frames_dither(dspfft_plan fwd, dspfft_plan inv, const uint8_t *d_in, uint8_t *d_out, float *d_work, double scalefactor,
                                                                double normalization, const dspfft_motion_filter_params *fp, const dspfft_motion_packed *packed,
                                                                unsigned long long *d_coeffs_coded, void *stream)
{
	if (!fwd || !inv || !d_in || !d_out) return fail(-1, "%s: null plan or buffer", kPackedFramesDither);
	if (!d_work) return fail(-1, "%s: null float work buffer (frames * h * w * components floats)", kPackedFramesDither);
	if (!packed) return fail(-1, "%s: null dspfft_motion_packed", kPackedFramesDither);
	if (fwd->f64 || inv->f64) return fail(-1, "%s takes f32 plans", kPackedFramesDither);
	if (!(scalefactor > 0) || !(normalization > 0) || !std::isfinite(scalefactor) || !std::isfinite(normalization))
		return fail(-1, "%s: scalefactor and normalization must be finite and > 0", kPackedFramesDither);
	RtCall c = {};
	c.fwd = fwd; c.inv = inv; c.d_in8 = d_in; c.d_out = d_work; c.dither = Dither{d_out, scalefactor, normalization}; c.fp = fp; c.packed = packed; c.packed_frames = true;
	c.coded = d_coeffs_coded; c.stream = stream;
	return roundtrip_core(c);
}

// motion_dither.hip's kernels with a pixel step.  Here, not beside dspfft_motion_dither_u8: the CPU emulation library has the entry and answers -3.
extern "C" int dspfft_motion_dither_u8_packed(uint8_t *d_pix, const float *d_coeffs, const dspfft_dither_geom *g, int components, double scalefactor, double normalization,
                                              int trc, void *stream)
{
	if (components < 2 || components > PACKED_MAX_COMPS) return fail(-1, "dither on packed pixels: components must be 2, 3 or 4 values per pixel, got %d (one component is dspfft_motion_dither_u8)", components);
	if (trc && !trc_built(trc)) return fail(-1, "dither on packed pixels: the transfer characteristic is not built");
	if (!dspfft_dither_packed_launch) return fail(-3, "dither on packed pixels: not built into this library (the kernels are HIP-only, motion_dither.hip)");
	char err[256] = "";
	if (dspfft_dither_packed_launch(d_pix, d_coeffs, g, components, scalefactor, normalization, trc, nullptr, 0, stream, err, sizeof err)) return fail(-1, "%s", err);
	return 0;
}

// ... over a rescaled block grid (rt_packed_grid): out of place, no work buffer, no coefficient limit
extern "C" int dspfft_execute_roundtrip_u8_packed_rescale(dspfft_plan fwd, dspfft_plan inv, const uint8_t *d_in, uint8_t *d_out, double out_mul,
                                                          const dspfft_motion_filter_params *fp, const dspfft_motion_packed *packed,
                                                          unsigned long long *d_coeffs_coded, void *stream)
{
	if (!fwd || !inv || !d_in || !d_out) return fail(-1, "%s: null plan or buffer", kPackedGrid);
	if (!packed) return fail(-1, "%s: null dspfft_motion_packed", kPackedGrid);
	if (fwd->f64 || inv->f64) return fail(-1, "%s takes f32 plans", kPackedGrid);
	RtCall c = {};
	c.fwd = fwd; c.inv = inv; c.d_in8 = d_in; c.d_out8 = d_out; c.mul8 = out_mul; c.fp = fp; c.packed = packed; c.packed_rescale = true;
	c.coded = d_coeffs_coded; c.stream = stream;
	return roundtrip_core(c);
}

// ... with motion --coeff-limit (block_rescale_packed_limit.hip): cl->d_work and cl->work_bytes are not read
extern "C" int dspfft_execute_roundtrip_u8_packed_rescale_limit(dspfft_plan fwd, dspfft_plan inv, const uint8_t *d_in, uint8_t *d_out, double out_mul,
                                                                const dspfft_motion_filter_params *fp, const dspfft_motion_packed *packed, const dspfft_coeff_limit *cl,
                                                                unsigned long long *d_coeffs_coded, void *stream)
{
	const char *const what = kPackedGridLimit;
	if (!fwd || !inv || !d_in || !d_out) return fail(-1, "%s: null plan or buffer", what);
	if (!packed) return fail(-1, "%s: null dspfft_motion_packed", what);
	if (fwd->f64 || inv->f64) return fail(-1, "%s takes f32 plans", what);
	if (!cl) return fail(-1, "%s: null dspfft_coeff_limit (dspfft_execute_roundtrip_u8_packed_rescale takes none)", what);
	if (!cl->keep) return fail(-1, "%s: keep must be at least 1 (dspfft_execute_roundtrip_u8_packed_rescale takes no limit)", what);
	if (!std::isfinite(cl->outside_mul) || !(cl->outside_mul > 0)) return fail(-1, "%s: outside_mul must be finite and > 0 (1 for motion's 3-D blocks)", what);
	RtCall c = {};
	c.fwd = fwd; c.inv = inv; c.d_in8 = d_in; c.d_out8 = d_out; c.mul8 = out_mul; c.fp = fp; c.packed = packed; c.packed_rescale = true;
	c.keep = cl->keep; c.outside_mul = cl->outside_mul;
	c.coded = d_coeffs_coded; c.stream = stream;
	return roundtrip_core(c);
}

// ... with motion's -d (block_rescale_packed_dither.hip: the kernel dithers in its tile and stores the bytes itself, so the call carries both d_out8
// and c.dither); cl NULL: no coefficient limit
extern "C" int dspfft_execute_roundtrip_u8_packed_rescale_dither(dspfft_plan fwd, dspfft_plan inv, const uint8_t *d_in, uint8_t *d_out, double scalefactor,
                                                                 double normalization, const dspfft_motion_filter_params *fp, const dspfft_motion_packed *packed,
                                                                 const dspfft_coeff_limit *cl, unsigned long long *d_coeffs_coded, void *stream)
{
	const char *const what = kPackedGridDither;
	if (!fwd || !inv || !d_in || !d_out) return fail(-1, "%s: null plan or buffer", what);
	if (!packed) return fail(-1, "%s: null dspfft_motion_packed", what);
	if (fwd->f64 || inv->f64) return fail(-1, "%s takes f32 plans", what);
	if (cl && !cl->keep) return fail(-1, "%s: coefficient limit: keep must be at least 1 (pass NULL for no limit)", what);
	if (cl && (!std::isfinite(cl->outside_mul) || !(cl->outside_mul > 0))) return fail(-1, "%s: coefficient limit: outside_mul must be finite and > 0 (1 for motion's 3-D blocks)", what);
	if (!(scalefactor > 0) || !(normalization > 0) || !std::isfinite(scalefactor) || !std::isfinite(normalization))
		return fail(-1, "%s: scalefactor and normalization must be finite and > 0", what);
	RtCall c = {};
	c.fwd = fwd; c.inv = inv; c.d_in8 = d_in; c.d_out8 = d_out; c.dither = Dither{d_out, scalefactor, normalization}; c.mul8 = scalefactor * normalization * normalization;
	c.fp = fp; c.packed = packed; c.packed_rescale = true;
	if (cl) { c.keep = cl->keep; c.outside_mul = cl->outside_mul; }
	c.coded = d_coeffs_coded; c.stream = stream;
	return roundtrip_core(c);
}

extern "C" int dspfft_scan_zigzag_frame_ids(uint32_t *d_ids, uint32_t w, uint32_t h, uint64_t step, void *s)
{
	if (!d_ids || !w || !h || !step) return fail(-1, "bad arguments");
	if ((uint64_t)w * h > 0xffffffffull) return fail(-1, "image too large for 32-bit offsets");
	return be_scan_zigzag_frame_ids(d_ids, w, h, step, s) ? fail(-4, "launch failed") : 0;
}

extern "C" int dspfft_plan_num_passes(dspfft_plan pl) { return pl ? (int)pl->passes.size() : 0; }

extern "C" int dspfft_execute_pass(dspfft_plan pl, int index, const float *d_in, float *d_out, void *stream)
{
	if (!pl || !d_in || !d_out || index < 0 || index >= (int)pl->passes.size()) return fail(-1, "bad plan, buffer or pass index");
	if (pl->f64) return fail(-1, "dspfft_execute_pass takes f32 plans");
	const std::vector<Pass> &passes = pick_passes(pl, d_in, d_out);
	const Pass &P = passes[index];
	return run_pass<float>(pl, P, P.first ? d_in : d_out, d_out, index + 1 == (int)passes.size(), stream);
}

// one pass over the items; items [timed_item, timed_item + timed_count) bracket each of their passes with pass_events (2 per pass).
// Buffers are float or double according to each item's plan.
template <class R>
static int execute_item(dspfft_plan pl, const void *in, void *out, void *st, bool timed, void *const *pass_events, int &ev)
{
	const R *d_in = (const R *)in;
	R *d_out = (R *)out;
	if (!timed) return execute_t<R>(pl, d_in, d_out, st);
	const std::vector<Pass> &passes = pick_passes(pl, d_in, d_out);
	for (size_t p = 0; p < passes.size(); p++) {
		const Pass &P = passes[p];
		if (be_event_record(pass_events[ev++], st)) return fail(-4, "event record failed");
		if (int rc = run_pass<R>(pl, P, P.first ? d_in : d_out, d_out, p + 1 == passes.size(), st)) return rc;
		if (be_event_record(pass_events[ev++], st)) return fail(-4, "event record failed");
	}
	return 0;
}
// double frames on more than one stream: the 3840 x 3 row pass goes back to one workgroup per line for the batch (backend.h)
struct ChanLinesGuard {
	bool on = false;
	ChanLinesGuard(int count, const dspfft_plan *plans, void *const *streams)
	{
		void *first = nullptr; bool have = false;
		for (int i = 0; streams && i < count && !on; i++) {
			if (!plans[i] || !plans[i]->f64) continue;
			if (!have) { first = streams[i]; have = true; } else if (streams[i] != first) on = true;
		}
		if (on) g_chan_lines_suspended++;
	}
	~ChanLinesGuard() { if (on) g_chan_lines_suspended--; }
};
// ---- forward/inverse pairs of a batch as one roundtrip ----
// Items i, i + 1 of a batch -- a forward plan, then its inverse in place on the forward's output, on the same stream -- are one roundtrip call
// without a filter: where rt_run_passes would run that call's two middle passes as one column kernel (rt_col_fused), the pair runs through it,
// the spectrum between the two column passes is never stored and the frame is swept three times instead of four.  The fused kernel is bit-identical
// to the pair pass by pass, so which repeats fuse (the timed ones do not: their passes are bracketed one by one) cannot be seen in the results.
// Checked once per call, not once per repeat: `calls[i]` is the checked call of the pair that begins at item i (fwd == NULL: none).
static std::atomic<unsigned long long> g_many_fused_pairs{0};
extern "C" unsigned long long dspfft_many_fused_pairs(void) { return g_many_fused_pairs.load(std::memory_order_relaxed); }
// what the listed fused column kernel of a tile keeps in LDS behind the tile (dct_spec.h ColSpecT::RT_TABLES: decided at compile time)
extern "C" unsigned long long dspfft_col_roundtrip_launches(void) { return g_col_roundtrip_launches.load(std::memory_order_relaxed); }
extern "C" long long dspfft_col_roundtrip_table_bytes(int N, int K, int T)
{
#define DSP_RT_TAB_ENTRY(n, k, t, ...) if (N == n && K == k && T == t) { typedef dspfft::ColSpec<n, k, t, __VA_ARGS__> S; return S::RT_TABLES ? (long long)S::RT_TAB_BYTES : 0; }
	DSPFFT_COL_SPECS(DSP_RT_TAB_ENTRY)
#undef DSP_RT_TAB_ENTRY
	return -1;
}

struct ManyPairs { std::vector<RtCall> calls; };
static bool many_pair_check(const dspfft_plan *plans, const void *const *d_in, void *const *d_out, void *const *streams, int i, RtCall &c)
{
	const dspfft_plan fwd = plans[i], inv = plans[i + 1];
	if (fwd->f64 || inv->f64 || (streams && streams[i] != streams[i + 1]) || d_out[i] != d_in[i + 1] || d_in[i + 1] != d_out[i + 1]) return false;
	// what dspfft_execute would run must be the plans' plain pass lists, which are what the roundtrip runs
	if (fwd->has_block || inv->has_block || &pick_passes(fwd, d_in[i], d_out[i]) != &fwd->passes || &pick_passes(inv, d_in[i + 1], d_out[i + 1]) != &inv->passes) return false;
	if (fwd->passes.empty() || inv->passes.empty()) return false;
	c = RtCall{};
	c.fwd = fwd; c.inv = inv; c.d_in = (const float *)d_in[i]; c.d_out = (float *)d_out[i]; c.stream = streams ? streams[i] : nullptr;
	char err[sizeof g_err];
	memcpy(err, g_err, sizeof err);                  // a pair that is none is no error of the batch
	const bool ok = rt_check(c) == 0 && !c.grid && !c.temporal && !c.block && !c.rescale;
	memcpy(g_err, err, sizeof err);
	if (!ok) return false;
	PassArgs af, ai;
	bool compiled;
	return rt_col_fused(c, fwd->passes.size() == 1 ? c.d_in : c.d_out, af, ai, compiled);
}
static void many_pairs_find(int count, const dspfft_plan *plans, const void *const *d_in, void *const *d_out, void *const *streams, ManyPairs &mp)
{
	mp.calls.clear();
	if (count < 2 || fused_roundtrip_off()) return;
	mp.calls.resize((size_t)count);
	bool any = false;
	for (int i = 0; i + 1 < count; i++) {
		RtCall c;
		if (many_pair_check(plans, d_in, d_out, streams, i, c)) { mp.calls[i] = c; any = true; } else mp.calls[i].fwd = nullptr;
	}
	mp.calls[count - 1].fwd = nullptr;
	if (!any) mp.calls.clear();
}

static int execute_many_once(int count, const dspfft_plan *plans, const void *const *d_in, void *const *d_out, void *const *streams,
                             int timed_item, int timed_count, void *const *pass_events, const ManyPairs &mp)
{
	ChanLinesGuard guard(count, plans, streams);
	int ev = 0;
	for (int i = 0; i < count; i++) {
		dspfft_plan pl = plans[i];
		void *st = streams ? streams[i] : nullptr;
		const bool timed = pass_events && i >= timed_item && i < timed_item + timed_count;
		// left to right, an item in one pair at most; a timed window that covers either item splits the pair
		if (!mp.calls.empty() && mp.calls[i].fwd && !timed && !(pass_events && i + 1 >= timed_item && i + 1 < timed_item + timed_count)) {
			if (int rc = rt_run_passes(mp.calls[i])) return rc;
			g_many_fused_pairs.fetch_add(1, std::memory_order_relaxed);
			i++;
			continue;
		}
		const int rc = pl->f64 ? execute_item<double>(pl, d_in[i], d_out[i], st, timed, pass_events, ev) : execute_item<float>(pl, d_in[i], d_out[i], st, timed, pass_events, ev);
		if (rc) return rc;
	}
	return 0;
}
static bool plan_is_staged(const dspfft_plan_s *pl)
{
	for (const Pass &P : pl->passes) if (P.tab.stage) return true;
	return false;
}
static int check_many(int count, const dspfft_plan *plans, const void *const *d_in, void *const *d_out, void *const *streams, int timed_item, int timed_count, bool events, bool f64_ok)
{
	if (count < 0 || (count && (!plans || !d_in || !d_out))) return fail(-1, "bad arguments");
	for (int i = 0; i < count; i++) {
		if (!plans[i] || !d_in[i] || !d_out[i]) return fail(-1, "item %d: null plan or buffer", i);
		if (plans[i]->f64 && !f64_ok) return fail(-1, "dspfft_execute_many takes f32 plans");
		// a staged DENSE pass (lines beyond what LDS holds) copies through ONE array owned by the plan: the same plan on two streams at once
		// would race on it
		if (streams && plan_is_staged(plans[i]))
			for (int j = 0; j < i; j++)
				if (plans[j] == plans[i] && streams[j] != streams[i]) return fail(-1, "items %d and %d: a plan with a staged pass (its lines pass through a device array of the plan) cannot run on two streams at once", j, i);
	}
	if (events) {
		if (timed_item < 0 || timed_count < 0 || timed_item + timed_count > count) return fail(-1, "timed items [%d, %d) lie outside the batch of %d", timed_item, timed_item + timed_count, count);
		// a one-pass small-block plan runs ONE fused kernel in dspfft_execute, not its axis passes: bracketing "passes" would time other kernels
		for (int i = timed_item; i < timed_item + timed_count; i++)
			if (plans[i]->has_block) return fail(-1, "item %d: per-pass events are not available for one-pass block plans", i);
	}
	return 0;
}

extern "C" int dspfft_execute_many(int count, const dspfft_plan *plans, const float *const *d_in, float *const *d_out, void *const *streams,
                                   int timed_item, int timed_count, void *const *pass_events)
{
	if (int rc = check_many(count, plans, (const void *const *)d_in, (void *const *)d_out, streams, timed_item, timed_count, pass_events != nullptr, false)) return rc;
	ManyPairs mp;
	many_pairs_find(count, plans, (const void *const *)d_in, (void *const *)d_out, streams, mp);
	return execute_many_once(count, plans, (const void *const *)d_in, (void *const *)d_out, streams, timed_item, timed_count, pass_events, mp);
}

// The frame loop of a clip inside the library: the batch `repeats` times (motion/motion.c:613-753 runs its per-frame plans once per
// frame of the clip, scan/scan.c:421-447 its inverse plan once per output frame).  See include/dspfft.h.
extern "C" int dspfft_execute_many_repeat(int count, const dspfft_plan *plans, const void *const *d_in, void *const *d_out, void *const *streams,
                                          int repeats, int rejoin_every, int timed_every, int timed_count, void *const *pass_events)
{
	if (repeats < 0 || rejoin_every < 0 || timed_every < 0) return fail(-1, "bad arguments");
	const bool ev = pass_events && timed_every > 0 && timed_count > 0;
	if (ev && count % timed_count) return fail(-1, "the timed window (%d items) must divide the batch (%d items)", timed_count, count);
	if (int rc = check_many(count, plans, d_in, d_out, streams, 0, ev ? count : 0, ev, true)) return rc;
	// distinct streams of the batch, in order of first use
	std::vector<void *> uniq;
	for (int i = 0; i < count; i++) { void *st = streams ? streams[i] : nullptr; if (std::find(uniq.begin(), uniq.end(), st) == uniq.end()) uniq.push_back(st); }
	std::vector<void *> join;
	const bool rejoin = rejoin_every > 0 && uniq.size() > 1;
	if (rejoin) for (size_t i = 0; i < uniq.size(); i++) { void *e = be_order_event_create(); if (!e) { for (void *x : join) be_event_destroy(x); return fail(-4, "event creation failed"); } join.push_back(e); }
	ManyPairs mp;
	if (repeats > 0) many_pairs_find(count, plans, d_in, d_out, streams, mp);
	int rc = 0, windows = 0;
	size_t ev_off = 0;
	for (int k = 0; k < repeats && !rc; k++) {
		if (rejoin && k && k % rejoin_every == 0) {
			// every stream waits for where every other stream stood at the end of the previous repeat: their relative phase cannot drift
			for (size_t a = 0; a < uniq.size() && !rc; a++) if (be_event_record(join[a], uniq[a])) rc = fail(-4, "event record failed");
			for (size_t a = 0; a < uniq.size() && !rc; a++)
				for (size_t b = 0; b < uniq.size() && !rc; b++)
					if (a != b && be_stream_wait_event(uniq[a], join[b])) rc = fail(-4, "stream wait failed");
			if (rc) break;
		}
		if (ev && k % timed_every == 0) {
			const int first = (int)(((long long)windows * timed_count) % count);
			rc = execute_many_once(count, plans, d_in, d_out, streams, first, timed_count, pass_events + ev_off, mp);
			for (int i = first; i < first + timed_count; i++) ev_off += 2 * pick_passes(plans[i], d_in[i], d_out[i]).size();    // (alignment of the pointers only)
			windows++;
		} else rc = execute_many_once(count, plans, d_in, d_out, streams, 0, 0, nullptr, mp);
	}
	for (void *x : join) be_event_destroy(x);
	return rc;
}
extern "C" void *dspfft_stream_create(void) { return be_stream_create(); }
extern "C" void dspfft_stream_destroy(void *s) { be_stream_destroy(s); }
extern "C" int dspfft_stream_synchronize(void *s) { return be_stream_synchronize(s) ? fail(-4, "stream synchronise failed") : 0; }
extern "C" void *dspfft_event_create(void) { return be_event_create(); }
extern "C" void dspfft_event_destroy(void *e) { be_event_destroy(e); }
extern "C" int dspfft_event_synchronize(void *e) { return e && !be_event_synchronize(e) ? 0 : fail(-4, "event synchronise failed"); }
extern "C" int dspfft_event_elapsed_ms(void *a, void *b, float *ms)
{
	if (!a || !b || !ms) return fail(-1, "bad arguments");
	return be_event_elapsed_ms(a, b, ms) ? fail(-4, "event query failed") : 0;
}

extern "C" void dspfft_destroy_plan(dspfft_plan pl)
{
	if (!pl) return;
	for (Pass &P : pl->passes) P.tab.release();
	for (Pass &P : pl->split) P.tab.release();
	if (pl->temporal) pl->temporal->tab.release();
	be_free(pl->zflags); be_free(pl->zpage); be_free(pl->zranges); be_free(pl->eids);
	if (pl->u8_tab_owned) be_free(pl->u8_tab);
	delete pl;
}

extern "C" int dspfft_plan_describe(dspfft_plan pl, char *buf, size_t buflen)
{
	if (!pl || !buf || !buflen) return fail(-1, "bad arguments");
	std::string s = std::string("backend ") + be_name() + "\n";
	// a split plan lists the passes dspfft_execute runs; the plain ones (masked / fused executions, unaligned buffers) follow
	for (const Pass &P : pl->split) { s += P.desc; s += "\n"; }
	if (pl->has_block) { s += pl->blk_desc; s += "\n"; }
	for (const Pass &P : pl->passes) { if (!pl->split.empty() || pl->has_block) s += "plain "; s += P.desc; if (!P.hostloop.empty()) s += " +hostloop"; s += "\n"; }
	if (pl->u8_trc) { s += "8-bit end of a roundtrip through transfer characteristic "; s += trc_name(pl->u8_trc); s += "\n"; }
	std::lock_guard<std::mutex> lock(pl->rt_mutex);                  // (another thread's first roundtrip over a clip may be adding to rt_slices)
	for (const auto &r : pl->rt_slices) {                            // (present once dspfft_execute_roundtrip_u8 has walked a clip in slices)
		char b[256];
		snprintf(b, sizeof b, "roundtrip_u8 in slices of %d frames (last: %d) on %d stream(s): ", r->frames, r->fwd_rem ? r->fwd_rem->howmany : r->frames, r->side ? 2 : 1);
		s += b; s += r->fwd->passes.back().desc; s += "\n";
	}
	snprintf(buf, buflen, "%s", s.c_str());
	return 0;
}

extern "C" size_t dspfft_plan_algorithmic_bytes(dspfft_plan pl) { return pl ? pl->alg_bytes : 0; }
#undef g_plan_effort
extern "C" void dspfft_set_plan_effort(int effort) { g_plan_effort_default.store(effort < 0 ? 0 : effort, std::memory_order_relaxed); }
extern "C" int dspfft_get_plan_effort(void) { return t_plan_effort >= 0 ? t_plan_effort : g_plan_effort_default.load(std::memory_order_relaxed); }
extern "C" void dspfft_set_thread_plan_effort(int effort) { t_plan_effort = effort < 0 ? -1 : effort; }
extern "C" int dspfft_get_thread_plan_effort(void) { return t_plan_effort; }

extern "C" int dspfft_scan_zigzag(uint32_t *d_lin, uint32_t w, uint32_t h, uint64_t first, uint64_t count, void *s)
{
	if (!d_lin || !w || !h || first + count > (uint64_t)w * h) return fail(-1, "bad zigzag range");
	if ((uint64_t)w * h > 0xffffffffull) return fail(-1, "image too large for 32-bit offsets");
	return be_scan_zigzag(d_lin, w, h, first, count, s) ? fail(-4, "launch failed") : 0;
}
// ---- scan methods other than zigzag (scan_core.h) ----
#include "scan_core.h"
extern "C" uint64_t dspfft_scan_limit(int method, uint32_t w32, uint32_t h32)
{
	const uint64_t w = w32, h = h32;
	switch (method) {
	case SCANM_ROW: return h;
	case SCANM_COLUMN: return w;
	case SCANM_DIAGONAL: return w + h - 1;
	case SCANM_MIRROR: case SCANM_BOX: return std::max(w, h);
	case SCANM_IBOX: return std::min(w, h);
	case SCANM_RADIAL: case SCANM_IRADIAL: return rint_hypot(w - 1, h - 1) + 1;      // the farthest corner's bucket is the last one
	case SCANM_HORIZONTAL: case SCANM_VERTICAL: case SCANM_ZIGZAG: return w * h;
	default: return 0;
	}
}
extern "C" uint64_t dspfft_scan_max_interval(int method, uint32_t w32, uint32_t h32)
{
	const uint64_t w = w32, h = h32;
	switch (method) {
	case SCANM_ROW: return w;
	case SCANM_COLUMN: return h;
	case SCANM_DIAGONAL: return std::min(w, h);
	case SCANM_MIRROR: return std::min(w, h) * 2 - 1;
	case SCANM_BOX: case SCANM_IBOX: return w + h - 1;                                // limit_sum (scan_methods.c:23,496,502)
	case SCANM_HORIZONTAL: case SCANM_VERTICAL: case SCANM_ZIGZAG: return 1;
	default: return 0;                                                                // radial / iradial: no closed form (owner ids only)
	}
}
// entries per scan index in a coordinate list: max_interval, plus the one entry the reference's callers over-allocate (scan.c:346) and
// ibox needs (index 0 emits its corner twice: w + h coordinates against max_interval = w + h - 1)
extern "C" uint64_t dspfft_scan_coord_slots(int method, uint32_t w, uint32_t h)
{
	const uint64_t m = dspfft_scan_max_interval(method, w, h);
	return (method == SCANM_BOX || method == SCANM_IBOX) ? m + 1 : m;
}
static int scan_args_ok(const void *p, int method, uint32_t w, uint32_t h)
{
	if (!p || !w || !h || method < 0 || method >= SCANM_COUNT) return fail(-1, "bad scan arguments");
	if ((uint64_t)w * h > 0xfffffffeull) return fail(-1, "image too large for 32-bit offsets");
	return 0;
}
extern "C" int dspfft_scan_owner_index(uint32_t *d_index, int method, uint32_t w, uint32_t h, void *s)
{
	if (int rc = scan_args_ok(d_index, method, w, h)) return rc;
	if (method == SCANM_BOX) return fail(-2, "box has no single owner per pixel: use dspfft_scan_coords + dspfft_scan_stamp");
	if (method == SCANM_ZIGZAG) return be_scan_zigzag_frame_ids(d_index, w, h, 0, s) ? fail(-4, "launch failed") : 0;
	return be_scan_owner_index(d_index, method, w, h, 0, s) ? fail(-4, "launch failed") : 0;
}
extern "C" int dspfft_scan_frame_ids(uint32_t *d_ids, int method, uint32_t w, uint32_t h, uint64_t step, void *s)
{
	if (int rc = scan_args_ok(d_ids, method, w, h)) return rc;
	if (!step) return fail(-1, "step must be >= 1");
	if (method == SCANM_BOX) return fail(-2, "box has no single owner per pixel: use dspfft_scan_coords + dspfft_scan_stamp");
	if (method == SCANM_ZIGZAG) return be_scan_zigzag_frame_ids(d_ids, w, h, step, s) ? fail(-4, "launch failed") : 0;
	return be_scan_owner_index(d_ids, method, w, h, step, s) ? fail(-4, "launch failed") : 0;
}
extern "C" int dspfft_scan_coords(uint32_t *d_lin, int method, uint32_t w, uint32_t h, uint64_t first, uint64_t count, void *s)
{
	if (int rc = scan_args_ok(d_lin, method, w, h)) return rc;
	const uint64_t slots = dspfft_scan_coord_slots(method, w, h);
	if (!slots) return fail(-2, "radial / iradial have no closed-form coordinate lists: use dspfft_scan_frame_ids");
	if (first + count > dspfft_scan_limit(method, w, h)) return fail(-1, "scan index range out of bounds");
	if (method == SCANM_ZIGZAG) return be_scan_zigzag(d_lin, w, h, first, count, s) ? fail(-4, "launch failed") : 0;
	return be_scan_coords(d_lin, method, w, h, first, count, slots, s) ? fail(-4, "launch failed") : 0;
}
extern "C" int dspfft_scan_stamp(uint32_t *d_ids, const uint32_t *d_lin, uint64_t nslots, uint32_t frame_id, void *s)
{
	if (!d_ids || (!d_lin && nslots)) return fail(-1, "bad arguments");
	return be_scan_stamp(d_ids, d_lin, nslots, frame_id, s) ? fail(-4, "launch failed") : 0;
}
extern "C" int dspfft_scan_index_to_frame_ids(uint32_t *d_ids, uint64_t n, uint64_t step, void *s)
{
	if (!d_ids || !n || !step) return fail(-1, "bad arguments");
	return be_scan_index_to_frame_ids(d_ids, n, step, s) ? fail(-4, "launch failed") : 0;
}
extern "C" size_t dspfft_scan_magnitude_work_bytes(uint32_t w, uint32_t h) { return be_scan_magnitude_work_bytes(w, h); }
extern "C" int dspfft_scan_magnitude_index(uint32_t *d_index, const float *d_coeffs, uint32_t w, uint32_t h, int channels, double qfactor,
                                           void *d_work, size_t work_bytes, uint32_t *limit, void *s)
{
	if (!d_index || !d_coeffs || !d_work || !w || !h || channels < 1) return fail(-1, "bad arguments");
	if ((uint64_t)w * h > 0xfffffffeull) return fail(-1, "image too large for 32-bit offsets");
	if (work_bytes < be_scan_magnitude_work_bytes(w, h)) return fail(-1, "work buffer too small: dspfft_scan_magnitude_work_bytes");
	return be_scan_magnitude_index(d_index, d_coeffs, w, h, channels, qfactor, d_work, work_bytes, limit, s) ? fail(-4, "magnitude sort failed") : 0;
}

extern "C" int dspfft_scan_scatter(float *r, const float *c, const uint32_t *lin, uint64_t count, uint64_t npix, int ch, void *s)
{
	if (!r || !c || (!lin && count) || ch < 1) return fail(-1, "bad arguments");
	return be_scan_scatter(r, c, lin, count, npix, ch, s) ? fail(-4, "launch failed") : 0;
}
extern "C" int dspfft_accumulate(float *sum, const float *img, uint64_t len, void *s)
{
	if (!sum || !img) return fail(-1, "bad arguments");
	return be_accumulate(sum, img, len, s) ? fail(-4, "launch failed") : 0;
}
extern "C" int dspfft_broadcast_dc(float *sum, const float *c, uint64_t npix, int ch, void *s)
{
	if (!sum || !c || ch < 1) return fail(-1, "bad arguments");
	return be_broadcast_dc(sum, c, npix, ch, s) ? fail(-4, "launch failed") : 0;
}
extern "C" int dspfft_u8_to_f32(float *d, const uint8_t *src, uint64_t len, void *s)
{
	if (!d || !src) return fail(-1, "bad arguments");
	return be_u8_to_f32(d, src, len, s) ? fail(-4, "launch failed") : 0;
}
extern "C" int dspfft_f32_to_u8(uint8_t *d, const float *src, double mul, uint64_t len, void *s)
{
	if (!d || !src) return fail(-1, "bad arguments");
	return be_f32_to_u8(d, src, mul, len, s) ? fail(-4, "launch failed") : 0;
}

// ---- motion --linear on 8-bit samples (include/dspfft.h; trc_u8_core.h; kernels in motion_ops.hip and the units named at the weak references) ----
extern "C" int dspfft_plan_set_u8_trc(dspfft_plan pl, int trc)
{
	if (!pl) return fail(-1, "null plan");
	if (trc == 0) {                      // back to the plain conversions; the tables go with the plan, or with the next function
		pl->u8_trc = 0;
		return 0;
	}
	if (pl->f64) return fail(-1, "8-bit transfer characteristic: the 8-bit roundtrip takes f32 plans");
	if (!trc_built(trc)) return fail(-1, "8-bit transfer characteristic %d is not built", trc);
	if (!dspfft_u8_trc_flat_launch || !dspfft_u8_trc_region_launch || !dspfft_dither_trc_launch || !dspfft_block_trc_launch || !dspfft_row_u8_trc_launch)
		return fail(-3, "8-bit transfer characteristic: not in this build (the kernels are HIP-only)");
	if (pl->u8_trc == trc) return 0;
	// fresh memory for another function's tables: a roundtrip enqueued earlier may still be reading the old ones (be_free waits for it)
	auto host = std::make_unique<TrcU8Tab>();
	trc_u8_tab_build(*host, trc);
	void *d = be_alloc(sizeof(TrcU8Tab));
	if (!d || be_upload(d, host.get(), sizeof(TrcU8Tab))) { be_free(d); return fail(-4, "8-bit transfer characteristic: table upload failed"); }
	if (pl->u8_tab_owned) be_free(pl->u8_tab);
	pl->u8_tab = d; pl->u8_tab_owned = true; pl->u8_trc = trc;
	return 0;
}
namespace {
int u8_trc_args(const void *dst, const void *src, int trc)
{
	if (!dst || !src) return fail(-1, "8-bit transfer characteristic: null buffer");
	if (!trc_built(trc)) return fail(-1, "8-bit transfer characteristic %d is not built", trc);
	if (!dspfft_u8_trc_flat_launch || !dspfft_u8_trc_region_launch) return fail(-3, "8-bit transfer characteristic: not in this build (the kernels are HIP-only, motion_ops.hip)");
	return 0;
}
int motion_u8_linear(void *d_dst, const void *d_src, const int n[3], const int minbuf_hw[2], int store, double scalefactor, double normalization, int trc, void *stream)
{
	if (!d_dst || !d_src || !n || !minbuf_hw || n[0] < 1 || n[1] < 1 || n[2] < 1 || minbuf_hw[0] < n[1] || minbuf_hw[1] < n[2]) return fail(-1, "motion --linear: bad arguments");
	if (int rc = u8_trc_args(d_dst, d_src, trc)) return rc;
	const long long st[3] = {(long long)minbuf_hw[0] * minbuf_hw[1], minbuf_hw[1], 1};
	return dspfft_u8_trc_region_launch(d_dst, d_src, n, st, st, store, scalefactor, normalization, normalization, trc, nullptr, stream) ? fail(-4, "motion --linear: kernel launch failed") : 0;
}
}  // namespace
extern "C" int dspfft_u8_to_f32_trc(float *d_dst, const uint8_t *d_src, uint64_t len, int trc, void *stream)
{
	if (int rc = u8_trc_args(d_dst, d_src, trc)) return rc;
	return dspfft_u8_trc_flat_launch(d_dst, d_src, 1.0, len, 0, trc, nullptr, stream) ? fail(-4, "8-bit transfer characteristic: kernel launch failed") : 0;
}
extern "C" int dspfft_f32_to_u8_trc(uint8_t *d_dst, const float *d_src, double mul, uint64_t len, int trc, void *stream)
{
	if (int rc = u8_trc_args(d_dst, d_src, trc)) return rc;
	return dspfft_u8_trc_flat_launch(d_dst, d_src, mul, len, 1, trc, nullptr, stream) ? fail(-4, "8-bit transfer characteristic: kernel launch failed") : 0;
}
extern "C" int dspfft_motion_load_u8_linear(float *d_coeffs, const uint8_t *d_pix, const int n[3], const int minbuf_hw[2], int trc, void *stream)
{
	return motion_u8_linear(d_coeffs, d_pix, n, minbuf_hw, 0, 1.0, 1.0, trc, stream);
}
extern "C" int dspfft_motion_store_u8_linear(uint8_t *d_pix, const float *d_coeffs, const int n[3], const int minbuf_hw[2], double scalefactor, double normalization,
                                             int trc, void *stream)
{
	return motion_u8_linear(d_pix, d_coeffs, n, minbuf_hw, 1, scalefactor, normalization, trc, stream);
}

// ---- transfer characteristics (include/dspfft.h; trc_core.h; kernels in pointwise.hip and motion_ops.hip) ----
extern "C" int dspfft_trc_from_name(const char *name) { return trc_from_name(name); }
extern "C" const char *dspfft_trc_name(int trc) { return trc_name(trc); }
extern "C" int dspfft_trc_apply_f32(float *d_dst, const float *d_src, uint64_t len, int trc, int inverse, void *stream)
{
	if (!d_dst || !d_src) return fail(-1, "transfer characteristic: null buffer");
	if (!trc_built(trc)) return fail(-1, "transfer characteristic %d is not built", trc);
	if (!dspfft_trc_apply_launch) return fail(-3, "transfer characteristic: not in this build (the kernel is HIP-only, pointwise.hip)");
	if (!len) return 0;
	return dspfft_trc_apply_launch(d_dst, d_src, len, trc, !!inverse, stream) ? fail(-4, "transfer characteristic: kernel launch failed") : 0;
}
namespace {
int motion_linear(float *d_dst, const float *d_src, const int n[3], const int minbuf_hw[2], int store, double scalefactor, double normalization, int trc, void *stream)
{
	if (!d_dst || !d_src || !n || !minbuf_hw || n[0] < 1 || n[1] < 1 || n[2] < 1 || minbuf_hw[0] < n[1] || minbuf_hw[1] < n[2]) return fail(-1, "motion --linear: bad arguments");
	if (!trc_built(trc)) return fail(-1, "motion --linear: transfer characteristic %d is not built", trc);
	if (!dspfft_motion_linear_launch) return fail(-3, "motion --linear: not in this build (the kernels are HIP-only, motion_ops.hip)");
	return dspfft_motion_linear_launch(d_dst, d_src, n, minbuf_hw, store, scalefactor, normalization, trc, stream) ? fail(-4, "motion --linear: kernel launch failed") : 0;
}
}  // namespace
extern "C" int dspfft_motion_load_f32_linear(float *d_coeffs, const float *d_pix, const int n[3], const int minbuf_hw[2], int trc, void *stream)
{
	return motion_linear(d_coeffs, d_pix, n, minbuf_hw, 0, 1.0, 1.0, trc, stream);
}
extern "C" int dspfft_motion_store_f32_linear(float *d_pix, const float *d_coeffs, const int n[3], const int minbuf_hw[2], double scalefactor, double normalization,
                                              int trc, void *stream)
{
	return motion_linear(d_pix, d_coeffs, n, minbuf_hw, 1, scalefactor, normalization, trc, stream);
}

// ---- scan's output frames (include/dspfft.h "scan's output frames on the device"; kernels in scan_frame.hip) ----
struct dspfft_scanframes_s {
	dspfft_scan_frame_opts o;
	uint32_t w, h;
	SfState *state;
	void *partials;
	uint32_t *flags;
	uint32_t *saved;                        // the last current coordinate list (bottom-right marks to clear)
	uint64_t saved_cap, saved_n;
	int trc;                                // scan -g: the left-hand panels' transfer characteristic, 0 none
	int prev;                               // what the last current mark lit: 0 nothing, 1 a range of prev_owner, 2 the saved list
	uint32_t prev_lo, prev_hi;
	const uint32_t *prev_owner;
};
namespace {
SfOp sf_op(dspfft_scanframes sf, int op, void *stream)
{
	SfOp o;
	memset(&o, 0, sizeof o);
	o.op = op; o.w = sf->w; o.h = sf->h;
	o.visualize = sf->o.visualize; o.spectrogram = sf->o.spectrogram; o.intermediates = sf->o.intermediates;
	o.max_intermediates = sf->o.max_intermediates; o.parity_depth = sf->o.parity_depth;
	o.scaletype = sf->o.spec_scaletype; o.signtype = sf->o.spec_signtype; o.gain = sf->o.spec_gain; o.trc = sf->trc;
	o.state = sf->state; o.partials = sf->partials; o.flags = sf->flags; o.stream = stream;
	return o;
}
int sf_run(SfOp &o)
{
	char err[256] = "";
	if (!dspfft_scanframes_launch) return fail(-3, "scan frames: not in this build (the kernels are HIP-only, scan_frame.hip)");
	return dspfft_scanframes_launch(&o, err, sizeof err) ? fail(-4, "%s", err) : 0;
}
// clears the bottom-right marks of the last current call (before the next one lights its own), unless `owner` can do it in its own pass
int sf_clear_prev(dspfft_scanframes sf, float *frame, const uint32_t *owner, void *stream)
{
	if (sf->prev == 2) {
		SfOp o = sf_op(sf, SF_OP_MARK_COORDS, stream);
		o.frame = frame; o.lin = sf->saved; o.nslots = sf->saved_n;
		if (int rc = sf_run(o)) return rc;
	} else if (sf->prev == 1 && sf->prev_owner != owner) {
		SfOp o = sf_op(sf, SF_OP_MARK_RANGE, stream);
		o.frame = frame; o.owner = sf->prev_owner; o.clo = sf->prev_lo; o.chi = sf->prev_hi; o.bottom = 1;
		if (int rc = sf_run(o)) return rc;
	}
	if (sf->prev != 1 || sf->prev_owner != owner) sf->prev = 0;
	return 0;
}
}  // namespace

extern "C" int dspfft_scanframes_create(dspfft_scanframes *out, uint32_t w, uint32_t h, const dspfft_scan_frame_opts *opts)
{
	if (!out || !opts || !w || !h) return fail(-1, "scan frames: bad arguments");
	*out = nullptr;
	if ((uint64_t)w * h > 0xfffffffeull) return fail(-1, "scan frames: image too large for 32-bit pixel indices");
	dspfft_scan_frame_opts o = *opts;
	if (o.spec_scaletype < SF_SCALE_NONE || o.spec_scaletype > SF_SCALE_LOG) return fail(-1, "scan frames: spec_scaletype must be 0..2");
	if (o.spec_signtype < SF_SIGN_NONE || o.spec_signtype > SF_SIGN_SATURATE) return fail(-1, "scan frames: spec_signtype must be 0..3");
	if (o.parity_depth < 0 || (o.parity_depth > 16 && o.parity_depth != 32)) return fail(-1, "scan frames: parity_depth must be 0, 1..16 or 32");
	if (!isfinite(o.spec_gain)) return fail(-1, "scan frames: spec_gain must be finite");
	o.visualize = o.visualize || o.spectrogram; o.spectrogram = !!o.spectrogram; o.visualize = !!o.visualize;       // scan.c:179-180: -s implies -v
	o.intermediates = o.intermediates || o.max_intermediates; o.intermediates = !!o.intermediates;                   // scan.c:186: -M implies -i
	o.max_intermediates = !!o.max_intermediates;
	if (o.spec_gain == 0) o.spec_gain = sf_default_gain(w, h);                                                        // scan.c:367-368
	dspfft_scanframes sf = new dspfft_scanframes_s();
	sf->o = o; sf->w = w; sf->h = h;
	if (dspfft_scanframes_launch) {                          // without the kernels (CPU emulation build) every later call reports it
		SfOp a = sf_op(sf, SF_OP_ALLOC, nullptr);
		if (int rc = sf_run(a)) { delete sf; return rc; }
		sf->state = a.state; sf->partials = a.partials; sf->flags = a.flags;
	}
	*out = sf;
	return 0;
}
extern "C" size_t dspfft_scanframes_frame_floats(dspfft_scanframes sf)
{
	if (!sf) return 0;
	return 3ull * sf->w * (1 + sf->o.visualize) * sf->h * (1 + sf->o.intermediates);
}
extern "C" int dspfft_scanframes_begin(dspfft_scanframes sf, float *d_frame, const float *d_coeffs, void *stream)
{
	if (!sf || !d_frame || !d_coeffs) return fail(-1, "scan frames: bad arguments");
	SfOp o = sf_op(sf, SF_OP_BEGIN, stream);
	o.frame = d_frame; o.coeffs = d_coeffs;
	sf->prev = 0;
	return sf_run(o);
}
extern "C" int dspfft_scanframes_mark_range(dspfft_scanframes sf, float *d_frame, const float *d_coeffs, const uint32_t *d_owner, uint32_t lo, uint32_t hi,
                                            int current, void *stream)
{
	if (!sf || !d_frame || !d_coeffs || !d_owner || lo > hi) return fail(-1, "scan frames: bad arguments");
	if (!sf->o.visualize) return 0;                          // scan.c:397,432: nothing lit without -v
	const bool bottom = current && sf->o.intermediates;
	SfOp o = sf_op(sf, SF_OP_MARK_RANGE, stream);
	o.frame = d_frame; o.coeffs = d_coeffs; o.owner = d_owner; o.lo = lo; o.hi = hi; o.top = 1; o.bottom = bottom;
	if (bottom) {
		if (int rc = sf_clear_prev(sf, d_frame, d_owner, stream)) return rc;
		if (sf->prev == 1) { o.clo = sf->prev_lo; o.chi = sf->prev_hi; }
	}
	if (int rc = sf_run(o)) return rc;
	if (bottom) { sf->prev = 1; sf->prev_lo = lo; sf->prev_hi = hi; sf->prev_owner = d_owner; }
	return 0;
}
extern "C" int dspfft_scanframes_mark_coords(dspfft_scanframes sf, float *d_frame, const float *d_coeffs, const uint32_t *d_lin, uint64_t nslots,
                                             int current, void *stream)
{
	if (!sf || !d_frame || !d_coeffs || (!d_lin && nslots)) return fail(-1, "scan frames: bad arguments");
	if (!sf->o.visualize) return 0;
	const bool bottom = current && sf->o.intermediates;
	if (bottom) {
		if (int rc = sf_clear_prev(sf, d_frame, nullptr, stream)) return rc;
	}
	SfOp o = sf_op(sf, SF_OP_MARK_COORDS, stream);
	o.frame = d_frame; o.coeffs = d_coeffs; o.lin = d_lin; o.nslots = nslots; o.top = 1; o.bottom = bottom;
	if (int rc = sf_run(o)) return rc;
	if (bottom) {
		SfOp c = sf_op(sf, SF_OP_SAVE_COORDS, stream);
		c.lin = d_lin; c.nslots = nslots; c.saved = &sf->saved; c.saved_cap = &sf->saved_cap;
		if (int rc = sf_run(c)) { sf->prev = 0; return rc; }
		sf->prev = 2; sf->saved_n = nslots;
	}
	return 0;
}
extern "C" int dspfft_scanframes_compose(dspfft_scanframes sf, float *d_frame, float *d_sum, float *d_image, const float *d_coeffs, const float *d_original,
                                         uint64_t frame, void *stream)
{
	if (!sf || !d_frame || !d_sum || !d_coeffs) return fail(-1, "scan frames: bad arguments");
	if (sf->o.intermediates && !d_image) return fail(-1, "scan frames: -i needs this frame's image (d_image)");
	if (sf->o.parity_depth && !d_original) return fail(-1, "scan frames: -P needs the original image (d_original)");
	SfOp o = sf_op(sf, SF_OP_COMPOSE, stream);
	o.frame = d_frame; o.sum = d_sum; o.image = d_image; o.coeffs = d_coeffs; o.original = sf->o.parity_depth ? d_original : nullptr; o.frame_no = frame;
	return sf_run(o);
}
extern "C" int dspfft_scanframes_set_trc(dspfft_scanframes sf, int trc)
{
	if (!sf) return fail(-1, "scan frames: bad arguments");
	if (trc && !trc_built(trc)) return fail(-1, "scan frames: transfer characteristic %d is not built", trc);
	sf->trc = trc;
	return 0;
}
extern "C" int dspfft_scanframes_parity(dspfft_scanframes sf, uint64_t *first_frame, void *stream)
{
	if (!sf || !first_frame) return fail(-1, "scan frames: bad arguments");
	if (!sf->o.parity_depth) return fail(-1, "scan frames: parity is not measured (parity_depth 0)");
	SfOp o = sf_op(sf, SF_OP_PARITY, stream);
	o.parity_out = first_frame;
	return sf_run(o);
}
extern "C" void dspfft_scanframes_destroy(dspfft_scanframes sf)
{
	if (!sf) return;
	if (dspfft_scanframes_launch) {
		SfOp o = sf_op(sf, SF_OP_FREE, nullptr);
		o.saved = &sf->saved;
		sf_run(o);
	}
	delete sf;
}
