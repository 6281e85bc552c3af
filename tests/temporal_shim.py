"""TEST INFRASTRUCTURE ONLY: the temporal block kernel's phases (dspfun_amd/csrc/temporal_core.h) compiled with g++ and walked thread by
thread -- a shim that builds the arguments the engine derives (the planner's radix order, the column pass's tables).  Shared by
tests/test_motion_temporal_cpu.py and tests/test_lengths_cpu.py: both import the `core` fixture and `run_core` from here."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import motion_ref as mr
from dspfun_amd.engine import Plan

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "dspfun_amd", "csrc")
HOLD = int(re.search(r"TEMPORAL_HOLD\s*=\s*(\d+)", open(os.path.join(CSRC, "temporal_core.h")).read()).group(1))

CPP = r'''
#include <stdint.h>
#include <math.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "temporal_core.h"
#include "../../include/dspfft.h"
using namespace dspfft;
// engine.cpp's factorize: fewest stages, then the smallest sum of radices, largest radix last
static const int kRadices[] = {16, 15, 13, 12, 11, 10, 9, 8, 7, 6, 5, 4, 3, 2};
static bool fsearch(int L, int depth, int maxdepth, std::vector<int> &cur, std::vector<int> &best, int &bestsum, int minr)
{
	if (L == 1) {
		int s = 0; for (int r : cur) s += r;
		if (best.empty() || cur.size() < best.size() || (cur.size() == best.size() && s < bestsum)) { best = cur; bestsum = s; }
		return true;
	}
	if (depth == maxdepth) return false;
	bool ok = false;
	for (int r : kRadices) {
		if (r > minr || L % r) continue;
		cur.push_back(r);
		ok |= fsearch(L / r, depth + 1, maxdepth, cur, best, bestsum, r);
		cur.pop_back();
	}
	return ok;
}
struct Tab { FftDesc F; std::vector<uint32_t> pos; std::vector<cx<float>> T, W; };
static bool tables(int N, Tab &t)
{
	std::vector<int> rad;
	for (int md = 1; md <= 8 && rad.empty(); md++) { std::vector<int> cur, best; int bs = 0; if (fsearch(N, 0, md, cur, best, bs, 16)) { std::sort(best.begin(), best.end()); rad = best; } }
	if (rad.empty()) return false;
	memset(&t.F, 0, sizeof t.F);
	t.F.L = N; t.F.ns = (int)rad.size();
	int Lc = N;
	for (int i = 0; i < t.F.ns; i++) { StageDesc &S = t.F.st[i]; S.R = rad[i]; S.Lc = Lc; S.M1 = Lc / rad[i]; S.twstep = N / Lc; S.divM1 = motion_filter_div((uint32_t)S.M1); Lc = S.M1; }
	t.pos.assign(N, 0);
	for (int p = 0; p < N; p++) {
		int rem = p, k = 0, mult = 1, span = N;
		for (int i = 0; i < t.F.ns; i++) { span /= rad[i]; int d = rem / span; rem -= d * span; k += d * mult; mult *= rad[i]; }
		t.pos[k] = (uint32_t)p;
	}
	const long double pi = 3.14159265358979323846264338327950288L;
	t.T.resize(N + 1); t.W.resize(N);
	for (int j = 0; j <= N; j++) t.T[j] = cmk<float>((float)cosl(pi * j / (2.0L * N)), (float)-sinl(pi * j / (2.0L * N)));
	for (int j = 0; j < N; j++) t.W[j] = cmk<float>((float)cosl(2 * pi * j / N), (float)-sinl(2 * pi * j / N));
	return true;
}
// the forward FFT's radices in the order the stages run, for the caller to compare with what the planner names
extern "C" int radices(int N, int *out)
{
	Tab t;
	if (!tables(N, t)) return -1;
	for (int i = 0; i < t.F.ns; i++) out[i] = t.F.st[i].R;
	return t.F.ns;
}
// in / out: float or 8-bit (the other NULL), [nd D][P] -> [nd S][P]; kforce: a narrower tile (0: the engine's choice)
extern "C" int run(const float *in, const uint8_t *in8, float *out, uint8_t *out8, int nd, int P, int D, int S, int kforce,
                   const dspfft_motion_filter_params *fp, double mul8, unsigned long long *coded)
{
	Tab tf, ti;
	if (!tables(D, tf) || !tables(S, ti)) return -1;
	const int m = D > S ? D : S;
	TemporalArgs a;
	memset((void *)&a, 0, sizeof a);
	int K = temporal_tile_k(m);
	if (!K) return -2;
	if (kforce && kforce < K) K = kforce;
	a.D = D; a.S = S; a.K = K; a.B = K / 2; a.P = P; a.ntiles = (P + K - 1) / K;
	a.blk_in = (long long)D * P; a.blk_out = (long long)S * P;
	a.in = in; a.in8 = in8; a.out = out; a.out8 = out8; a.mul8 = mul8;
	a.ff = tf.F; a.fi = ti.F; a.Tf = tf.T.data(); a.Wf = tf.W.data(); a.posf = tf.pos.data(); a.Ti = ti.T.data(); a.Wi = ti.W.data(); a.posi = ti.pos.data();
	// motion_temporal_plans' scales as the engine holds them (set through a float argument)
	const double r2 = sqrt(2.0);
	a.f_scale = (float)(2 * r2 * 2); a.f_in0 = 1.f; a.f_out0 = (float)(1 / r2); a.i_scale = (float)(2 / (2 * r2)); a.i_in0 = (float)r2; a.i_out0 = 1.f;
	if (fp) motion_filter_from(*fp, a.filt);
	a.divB = motion_filter_div((uint32_t)a.B); a.divQ = motion_filter_div((uint32_t)(K / 4)); a.div_tiles = motion_filter_div((uint32_t)a.ntiles);
	const int nthr = temporal_threads(m, K), nwg = a.ntiles * nd;
	if ((D / 2 + 1) * a.B > TEMPORAL_HOLD * nthr) return -3;
	const size_t nfl = temporal_tile_bytes(a) / sizeof(float);
	std::vector<float> raw(nfl + 8);
	cx<float> *buf = (cx<float> *)(((uintptr_t)raw.data() + 15) & ~(uintptr_t)15);
	std::vector<TemporalHeld> held(nthr);
	unsigned long long mine = 0;
	for (int wg = 0; wg < nwg; wg++) {
		long long bin, bout; int valid;
		temporal_base(a, (uint32_t)wg, bin, bout, valid);
		for (size_t i = 0; i < nfl; i++) ((float *)buf)[i] = NAN;        // what no phase writes must never reach a valid column
		for (int tid = 0; tid < nthr; tid++) temporal_phase_load(a, buf, bin, valid, tid, nthr, nullptr);
		for (int s = 0; s < a.ff.ns; s++) for (int tid = 0; tid < nthr; tid++) temporal_stage(a, buf, false, s, tid, nthr);
		for (int tid = 0; tid < nthr; tid++) temporal_post_read(a, buf, valid, tid, nthr, held[tid]);
		for (int tid = 0; tid < nthr; tid++) temporal_post_write(a, buf, valid, tid, nthr, held[tid], mine);
		for (int tid = 0; tid < nthr; tid++) temporal_pre(a, buf, valid, tid, nthr);
		for (int s = 0; s < a.fi.ns; s++) for (int tid = 0; tid < nthr; tid++) temporal_stage(a, buf, true, s, tid, nthr);
		for (int tid = 0; tid < nthr; tid++) temporal_phase_store(a, buf, bout, valid, tid, nthr, nullptr, 0);
	}
	if (coded) *coded += mine;
	return K * 1000 + nthr;
}
'''


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    d = tmp_path_factory.mktemp("temporal_core")
    src, so = d / "core.cpp", d / "core.so"
    src.write_text(CPP)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I", CSRC, str(src), "-o", str(so)])
    lib = C.CDLL(str(so))
    lib.run.argtypes = [C.c_void_p] * 4 + [C.c_int] * 5 + [C.c_void_p, C.c_double, C.c_void_p]
    lib.radices.argtypes = [C.c_int, C.c_void_p]
    return lib


def run_core(core, ref, D, S, u8=True, flt=None, kforce=0):
    """the clip ref["vol"] ([frames][H][W], 8-bit) through the shim -> (output clip, coded count, (tile width, threads))"""
    vol = ref["vol"]
    nd = vol.shape[0] // D
    hw = vol.shape[1:]
    src = np.ascontiguousarray(vol if u8 else vol.astype(np.float32))
    out = np.full((nd * S,) + hw, 9, dtype=np.uint8 if u8 else np.float32)
    coded = np.zeros(1, dtype=np.uint64)
    sf, nm = mr.consts((D, 1, 1), (S, 1, 1))
    fp = Plan._filter_params(flt)
    rc = core.run(None if u8 else src.ctypes.data, src.ctypes.data if u8 else None, None if u8 else out.ctypes.data, out.ctypes.data if u8 else None,
                  nd, int(np.prod(hw)), D, S, kforce, C.addressof(fp) if fp is not None else None, sf * nm * nm if u8 else 1.0, coded.ctypes.data)
    assert rc > 0, rc
    return out, int(coded[0]), divmod(rc, 1000)


def shim_radices(core, N):
    out = (C.c_int * 8)()
    n = core.radices(N, out)
    assert n > 0, N
    return list(out[:n])


def expected_tile(D, S):
    m = max(D, S)
    K = 128 if m <= 128 else 64 if m <= 256 else 32 if m <= 512 else 16
    return K, (512 if m * K > 8192 else 256)
