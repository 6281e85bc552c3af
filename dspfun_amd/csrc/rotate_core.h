// rotate_core.h -- rotate (motion/rotate.c:74-89, 159-164): a clip's three axes permuted, with flips, the index arithmetic and the phases of
// rotate.hip's kernels.  Input is [len[2]][len[1]][len[0]] elements of E = 1..4 bytes; output axis o runs over input axis map[o], and input
// axis a is read backwards iff invert[map[a]] (the reference's rule, 3-cycles included: RotArgs::flip is indexed by INPUT axis).
//
// Two shapes, chosen by where input x goes:
//   rows   map[0] == 0: every output row is one input row, possibly reversed.  A lane moves one 16-byte group of the OUTPUT row, stored at a
//          16-byte aligned address; its source bytes are loaded as one 16-byte vector at whatever address they have.  A reversed row reverses
//          the elements inside the vector in registers (a byte permute per dword and the dwords in reverse order).  E = 3 reversed: 16 bytes
//          hold no whole number of elements, so a lane takes 48 bytes (three aligned stores); the 16 or 17 elements they touch are 48 or 51
//          contiguous source bytes, loaded as three vectors and a dword, and every output dword is picked out of them by constants that depend
//          only on the row's phase (its aligned start modulo 3).  What lies before the first and after the last aligned group of a row is
//          moved byte by byte, one byte per lane.
//   tiles  map[0] == a != 0: a workgroup transposes a tile of the (x, a) plane at one b (the remaining axis) through LDS.
//          E = 1: a 128 x 128 byte tile.  A lane loads four dwords along x from four consecutive a rows, transposes the 4 x 4 bytes in
//          registers (eight byte permutes) and writes four dwords, each four consecutive a of one x, to the transposed tile T[x][a]; the
//          store phase reads T's rows as dwords and stores them at 4-byte aligned output addresses.  Where the output row's address is not
//          aligned, the dword is cut out of two neighbouring LDS dwords (alignbyte); a flip of a reads the window from the far end and
//          reverses its bytes.  Up to three bytes at either end of a row segment are stored singly.
//          LDS pitch.  T's rows are 128 bytes = 32 dwords.  The write of one instruction comes from 32 lanes with x = 4 xq + j (xq = 0..31) and
//          one a-quad aq: dword address x P + aq, bank (4 P xq + c) mod 32 for a pitch of P dwords.  4 P xq mod 32 takes at most 8 values, so NO
//          padding P makes this write conflict-free; the rows keep their 32 dwords (16 KB for the tile) and the dword column is swizzled
//          instead, col = aq ^ (x >> 2): the write's banks are aq ^ xq, all 32 distinct, and the store phase's 32 lanes read consecutive
//          columns d of one row x, banks d ^ (x >> 2), again distinct (LDS banks are counted per 32-lane half for 4-byte accesses).
//          E = 2, 3, 4: a 64 x 64 element tile, one element per lane and per LDS dword, T[a][x] at a pitch of 65 dwords: the load writes
//          consecutive x of one a (consecutive banks), the store reads one x of 32 consecutive a, banks (65 a + x) mod 32 = (a + x) mod 32,
//          distinct.  For E = 4 that is four bytes per lane along x on the way in and along a on the way out.
// Flips of x and b only change the output address of a tile's rows; b's place among the output axes only changes the strides.
// Plain C++17 for device (hipcc) and host (g++: tests/test_rotate_cpu.py walks every workgroup and lane).
#pragma once
#include <stdint.h>
#include <stddef.h>
#include "radix.h"

// the host walk counts stores through this (tests/test_rotate_cpu.py); nothing in the product
#ifndef ROT_NOTE_STORE
#define ROT_NOTE_STORE(p, n) ((void)0)
#endif

namespace dspfft {

enum {
	ROT_THREADS = 256,
	ROT_TILE_B = 128,          // E = 1: tile extent in bytes, both ways
	ROT_TILE_E = 64,           // E = 2..4: tile extent in elements, both ways
	ROT_PITCH_E = 65,          // ... and its pitch in dwords
	ROT_LDS_BYTES = ROT_TILE_E * ROT_PITCH_E * 4      // (>= 128 x 128)
};

struct alignas(16) RotVec { uint32_t v[4]; };

struct RotArgs {
	const unsigned char *in;
	unsigned char *out;
	uint64_t len[3];           // w, h, frames in elements
	int E, map[3], flip[3];    // flip[a]: input axis a is read backwards
	// rows
	uint64_t rb;               // bytes per row
	uint64_t orow[2];          // extents of output axes 1, 2
	int tpr;                   // threads per row, a power of two up to ROT_THREADS
	uint64_t nwg;              // workgroups, either shape
	// tiles
	int a, b;                  // the input axis that becomes output x, and the one left over
	int tile;                  // tile extent in elements
	uint64_t in_sa, in_sb;     // input strides of a and b, in elements
	uint64_t out_sx, out_sb;   // output strides of input x and b, in elements (a's is 1)
	uint64_t ntx, nta;         // tiles along x and a
};

DSP_HD bool rot_is_permutation(const int map[3])
{
	int seen = 0;
	for (int i = 0; i < 3; i++) { if (map[i] < 0 || map[i] > 2) return false; seen |= 1 << map[i]; }
	return seen == 7;
}

// derived geometry; len, E, map valid (the caller's checks)
DSP_HD void rot_setup(RotArgs &r, const uint64_t len[3], int E, const int map[3], const int invert[3])
{
	for (int i = 0; i < 3; i++) { r.len[i] = len[i]; r.map[i] = map[i]; }
	for (int i = 0; i < 3; i++) r.flip[i] = invert[map[i]] ? 1 : 0;
	r.E = E;
	r.rb = len[0] * (uint64_t)E;
	r.orow[0] = len[map[1]]; r.orow[1] = len[map[2]];
	r.a = map[0]; r.b = 0; r.tile = 0; r.in_sa = r.in_sb = r.out_sx = r.out_sb = r.ntx = r.nta = 0; r.tpr = 0;
	if (map[0] == 0) {
		const uint64_t groups = (r.rb + 15) / 16;
		int t = 16;
		while (t < ROT_THREADS && (uint64_t)t < groups) t <<= 1;
		r.tpr = t;
		const uint64_t rows = r.orow[0] * r.orow[1], per = (uint64_t)(ROT_THREADS / t);
		r.nwg = (rows + per - 1) / per;
		return;
	}
	r.b = 3 - r.a;
	r.tile = E == 1 ? ROT_TILE_B : ROT_TILE_E;
	r.in_sa = r.a == 1 ? len[0] : len[0] * len[1];
	r.in_sb = r.b == 1 ? len[0] : len[0] * len[1];
	if (map[1] == 0) { r.out_sx = len[r.a]; r.out_sb = len[r.a] * len[0]; }
	else { r.out_sb = len[r.a]; r.out_sx = len[r.a] * len[r.b]; }
	r.ntx = (len[0] + r.tile - 1) / r.tile;
	r.nta = (len[r.a] + r.tile - 1) / r.tile;
	r.nwg = r.ntx * r.nta * len[r.b];
}

// ---- byte shuffles: the device's instructions, restated for the host ----
DSP_HD uint32_t rot_perm(uint32_t hi, uint32_t lo, uint32_t sel)
{
#if defined(__HIP_DEVICE_COMPILE__)
	return __builtin_amdgcn_perm(hi, lo, sel);
#else
	const uint64_t both = ((uint64_t)hi << 32) | lo;
	uint32_t r = 0;
	for (int i = 0; i < 4; i++) r |= (uint32_t)((both >> (8 * ((sel >> (8 * i)) & 7))) & 0xffu) << (8 * i);
	return r;
#endif
}
// bytes s .. s + 3 of the eight bytes lo, hi
DSP_HD uint32_t rot_alignbyte(uint32_t hi, uint32_t lo, uint32_t s)
{
#if defined(__HIP_DEVICE_COMPILE__)
	return __builtin_amdgcn_alignbyte(hi, lo, s);
#else
	return (uint32_t)(((((uint64_t)hi) << 32) | lo) >> (8 * (s & 3)));
#endif
}
DSP_HD uint32_t rot_bswap(uint32_t v) { return rot_perm(0, v, 0x00010203u); }
// the elements of a dword in reverse order
template <int E> DSP_HD uint32_t rot_rev_dword(uint32_t v) { return E == 1 ? rot_bswap(v) : E == 2 ? rot_perm(0, v, 0x01000302u) : v; }

// rows r0..r3 of four bytes each -> columns: c[j] = {r0[j], r1[j], r2[j], r3[j]}
DSP_HD void rot_transpose4x4(const uint32_t r[4], uint32_t c[4])
{
	const uint32_t t0 = rot_perm(r[1], r[0], 0x05010400u), t1 = rot_perm(r[1], r[0], 0x07030602u);
	const uint32_t u0 = rot_perm(r[3], r[2], 0x05010400u), u1 = rot_perm(r[3], r[2], 0x07030602u);
	c[0] = rot_perm(u0, t0, 0x05040100u); c[1] = rot_perm(u0, t0, 0x07060302u);
	c[2] = rot_perm(u1, t1, 0x05040100u); c[3] = rot_perm(u1, t1, 0x07060302u);
}

template <int N> DSP_HD void rot_store_n(unsigned char *dst, const void *src)
{
	ROT_NOTE_STORE(dst, N);
	__builtin_memcpy(dst, src, N);
}
DSP_HD void rot_store_vec(unsigned char *dst, const RotVec &v)      // dst is 16-byte aligned
{
	ROT_NOTE_STORE(dst, 16);
	*reinterpret_cast<RotVec *>(dst) = v;
}

// =============================================== rows ===============================================
// output row -> byte offsets of the output row and of the input row it copies
DSP_HD void rot_row_offsets(const RotArgs &r, uint64_t row, uint64_t &out_off, uint64_t &in_off)
{
	const uint64_t o2 = row / r.orow[0], o1 = row - o2 * r.orow[0];
	uint64_t c[3] = {0, 0, 0};
	c[r.map[1]] = r.flip[r.map[1]] ? r.orow[0] - 1 - o1 : o1;
	c[r.map[2]] = r.flip[r.map[2]] ? r.orow[1] - 1 - o2 : o2;
	out_off = row * r.rb;
	in_off = (c[2] * r.len[1] + c[1]) * r.rb;
}
// a row at address dst: `head` single bytes up to the first 16-byte boundary, `ngroups` groups of G bytes, `tail` single bytes
DSP_HD void rot_row_split(uint64_t dst_addr, uint64_t rb, int G, int &head, uint64_t &ngroups, int &tail)
{
	uint64_t h = (0 - dst_addr) & 15;
	if (h > rb) h = rb;
	head = (int)h;
	ngroups = (rb - h) / (uint64_t)G;
	tail = (int)(rb - h - ngroups * (uint64_t)G);
}
// the source byte of output byte q of a row
DSP_HD uint64_t rot_row_src_byte(const RotArgs &r, uint64_t q, bool flip)
{
	if (!flip) return q;
	const uint64_t e = q / (uint64_t)r.E;
	return (r.len[0] - 1 - e) * (uint64_t)r.E + (q - e * (uint64_t)r.E);
}

// a reversed 48-byte group of 3-byte elements at output byte q = 3 e0 + F: elements e0 .. e0 + nel - 1 (nel = 16, or 17 when F != 0) are the
// contiguous source bytes [B, B + 3 nel), B = 3 (w - e0 - nel); output byte i is element k = (F + i) / 3, component (F + i) % 3, source byte
// 3 (nel - 1 - k) + component from B.  L[0..11]: source bytes 0..47; L[12]: source bytes 47..50 (F != 0 only).
template <int F> DSP_HD void rot_row_group_rev3(const RotArgs &r, const unsigned char *src_row, unsigned char *dst, uint64_t q)
{
	constexpr int nel = F ? 17 : 16;
	const uint64_t e0 = q / 3;
	const unsigned char *src = src_row + 3 * (r.len[0] - e0 - nel);
	uint32_t L[13];
	__builtin_memcpy(&L[0], src, 16); __builtin_memcpy(&L[4], src + 16, 16); __builtin_memcpy(&L[8], src + 32, 16);
	L[12] = 0;
	if (F) __builtin_memcpy(&L[12], src + 47, 4);
#pragma unroll
	for (int g = 0; g < 3; g++) {
		RotVec o;
#pragma unroll
		for (int d = 0; d < 4; d++) {
			uint32_t w = 0;
#pragma unroll
			for (int i = 0; i < 4; i++) {
				const int p = F + 16 * g + 4 * d + i, k = p / 3, off = 3 * (nel - 1 - k) + p % 3;
				const uint32_t byte = off < 48 ? (L[off >> 2] >> (8 * (off & 3))) & 0xffu : (L[12] >> (8 * (off - 47))) & 0xffu;
				w |= byte << (8 * i);
			}
			o.v[d] = w;
		}
		rot_store_vec(dst + 16 * g, o);
	}
}

// one 16-byte group (48 for reversed 3-byte elements) at output byte q of a row; dst = the group's (aligned) address
template <int E, bool FLIP> DSP_HD void rot_row_group(const RotArgs &r, const unsigned char *src_row, unsigned char *dst, uint64_t q)
{
	if constexpr (FLIP && E == 3) {
		switch ((int)(q % 3)) {
		case 0: rot_row_group_rev3<0>(r, src_row, dst, q); break;
		case 1: rot_row_group_rev3<1>(r, src_row, dst, q); break;
		default: rot_row_group_rev3<2>(r, src_row, dst, q); break;
		}
	} else {
		RotVec v;
		if constexpr (!FLIP) {
			__builtin_memcpy(&v, src_row + q, 16);
		} else {
			RotVec s;
			__builtin_memcpy(&s, src_row + (r.rb - q - 16), 16);
#pragma unroll
			for (int d = 0; d < 4; d++) v.v[d] = rot_rev_dword<E>(s.v[3 - d]);
		}
		rot_store_vec(dst, v);
	}
}

// everything thread `tid` of workgroup `wg` does
template <int E, bool FLIP> DSP_HD void rot_rows_thread(const RotArgs &r, uint64_t wg, int tid)
{
	constexpr int G = (FLIP && E == 3) ? 48 : 16;
	const int per = ROT_THREADS / r.tpr;
	const uint64_t row = wg * (uint64_t)per + (uint64_t)(tid / r.tpr);
	if (row >= r.orow[0] * r.orow[1]) return;
	uint64_t out_off, in_off;
	rot_row_offsets(r, row, out_off, in_off);
	unsigned char *dst = r.out + out_off;
	const unsigned char *src = r.in + in_off;
	int head, tail;
	uint64_t ngroups;
	rot_row_split((uint64_t)(uintptr_t)dst, r.rb, G, head, ngroups, tail);
	const uint64_t items = ngroups + (uint64_t)(head + tail);
	for (uint64_t it = (uint64_t)(tid & (r.tpr - 1)); it < items; it += (uint64_t)r.tpr) {
		if (it < ngroups) {
			const uint64_t q = (uint64_t)head + it * G;
			rot_row_group<E, FLIP>(r, src, dst + q, q);
		} else {
			const uint64_t e = it - ngroups;
			const uint64_t q = e < (uint64_t)head ? e : (uint64_t)head + ngroups * G + (e - (uint64_t)head);
			const unsigned char byte = src[rot_row_src_byte(r, q, FLIP)];
			rot_store_n<1>(dst + q, &byte);
		}
	}
}

// =============================================== tiles ===============================================
struct RotTile {
	uint64_t x0, a0, b;        // the tile's first x and a, its b
	int nx, na;                // valid extents (the last tile of an axis is short)
};

DSP_HD RotTile rot_tile_of(const RotArgs &r, uint64_t wg)
{
	RotTile t;
	const uint64_t rest = wg / r.ntx, tx = wg - rest * r.ntx;
	t.b = rest / r.nta;
	const uint64_t ta = rest - t.b * r.nta;
	t.x0 = tx * (uint64_t)r.tile; t.a0 = ta * (uint64_t)r.tile;
	const uint64_t rx = r.len[0] - t.x0, ra = r.len[r.a] - t.a0;
	t.nx = rx < (uint64_t)r.tile ? (int)rx : r.tile;
	t.na = ra < (uint64_t)r.tile ? (int)ra : r.tile;
	return t;
}
// byte offset of the tile's input row al (its element x0)
DSP_HD uint64_t rot_tile_in_row(const RotArgs &r, const RotTile &t, int al)
{
	return (t.x0 + r.in_sa * (t.a0 + (uint64_t)al) + r.in_sb * t.b) * (uint64_t)r.E;
}
// byte offset of the output row segment that the tile's column xl becomes: na elements along output x
DSP_HD uint64_t rot_tile_out_row(const RotArgs &r, const RotTile &t, int xl)
{
	const uint64_t x = t.x0 + (uint64_t)xl;
	const uint64_t ix = r.flip[0] ? r.len[0] - 1 - x : x;
	const uint64_t ib = r.flip[r.b] ? r.len[r.b] - 1 - t.b : t.b;
	const uint64_t oa = r.flip[r.a] ? r.len[r.a] - (t.a0 + (uint64_t)t.na) : t.a0;
	return (ix * r.out_sx + ib * r.out_sb + oa) * (uint64_t)r.E;
}
// position t of an output row segment reads the tile's a index ...
DSP_HD int rot_tile_a_of(const RotArgs &r, const RotTile &t, int pos) { return r.flip[r.a] ? t.na - 1 - pos : pos; }

// ---- E = 1: LDS dword index of bytes 4 d .. 4 d + 3 (along a) of the transposed tile's row x ----
DSP_HD int rot_lds_b(int x, int d) { return x * (ROT_TILE_B / 4) + (d ^ (x >> 2)); }
DSP_HD uint32_t rot_lds_byte(const uint32_t *lds, int x, int al) { return (lds[rot_lds_b(x, al >> 2)] >> (8 * (al & 3))) & 0xffu; }

// load: item = (a-quad aq, x-quad xq); 32 consecutive lanes take the 32 x-quads of one a-quad
DSP_HD void rot_tile_load_b(const RotArgs &r, const RotTile &t, uint32_t *lds, int tid)
{
	constexpr int Q = ROT_TILE_B / 4, PER = Q * Q / ROT_THREADS;
	uint32_t v[PER][4];
	// all loads of a thread before the first use
#pragma unroll
	for (int u = 0; u < PER; u++) {
		const int it = tid + u * ROT_THREADS, xq = it & (Q - 1), aq = it / Q;
#pragma unroll
		for (int i = 0; i < 4; i++) {
			const int al = 4 * aq + i;
			v[u][i] = 0;
			if (al < t.na && 4 * xq < t.nx) {
				const unsigned char *p = r.in + rot_tile_in_row(r, t, al) + 4 * xq;
				if (4 * xq + 4 <= t.nx) __builtin_memcpy(&v[u][i], p, 4);
				else for (int k = 0; 4 * xq + k < t.nx; k++) v[u][i] |= (uint32_t)p[k] << (8 * k);      // the row's last, short quad
			}
		}
	}
#pragma unroll
	for (int u = 0; u < PER; u++) {
		const int it = tid + u * ROT_THREADS, xq = it & (Q - 1), aq = it / Q;
		if (4 * aq >= t.na || 4 * xq >= t.nx) continue;
		uint32_t c[4];
		rot_transpose4x4(v[u], c);
#pragma unroll
		for (int j = 0; j < 4; j++) lds[rot_lds_b(4 * xq + j, aq)] = c[j];
	}
}

// store: 32 consecutive lanes take the 32 dwords of one output row segment; then the segments' unaligned ends, a byte per lane
DSP_HD void rot_tile_store_b(const RotArgs &r, const RotTile &t, const uint32_t *lds, int tid)
{
	constexpr int Q = ROT_TILE_B / 4;
	const bool fa = r.flip[r.a] != 0;
	for (int it = tid; it < ROT_TILE_B * Q; it += ROT_THREADS) {
		const int xl = it / Q, k = it & (Q - 1);
		if (xl >= t.nx) break;
		unsigned char *dst = r.out + rot_tile_out_row(r, t, xl);
		int h = (int)((0 - (uint64_t)(uintptr_t)dst) & 3);
		if (h > t.na) h = t.na;
		if (k >= (t.na - h) >> 2) continue;
		const int pos = h + 4 * k, ws = fa ? t.na - 4 - pos : pos, d = ws >> 2;
		const uint32_t lo = lds[rot_lds_b(xl, d)], hi = lds[rot_lds_b(xl, d + 1 < Q ? d + 1 : d)];
		uint32_t w = rot_alignbyte(hi, lo, (uint32_t)(ws & 3));
		if (fa) w = rot_bswap(w);
		rot_store_n<4>(dst + pos, &w);
	}
	for (int it = tid; it < ROT_TILE_B * 8; it += ROT_THREADS) {
		const int xl = it >> 3, e = it & 7;
		if (xl >= t.nx) break;
		unsigned char *dst = r.out + rot_tile_out_row(r, t, xl);
		int h = (int)((0 - (uint64_t)(uintptr_t)dst) & 3);
		if (h > t.na) h = t.na;
		const int nd = (t.na - h) >> 2;
		const int pos = e < 4 ? e : h + 4 * nd + (e - 4);
		if (e < 4 ? e >= h : pos >= t.na) continue;
		const unsigned char byte = (unsigned char)rot_lds_byte(lds, xl, rot_tile_a_of(r, t, pos));
		rot_store_n<1>(dst + pos, &byte);
	}
}

// ---- E = 2..4: an element per lane and per LDS dword ----
DSP_HD int rot_lds_e(int al, int xl) { return al * ROT_PITCH_E + xl; }

template <int E> DSP_HD void rot_tile_load_e(const RotArgs &r, const RotTile &t, uint32_t *lds, int tid)
{
	constexpr int T = ROT_TILE_E, PER = T * T / ROT_THREADS, BATCH = 8;
	for (int u0 = 0; u0 < PER; u0 += BATCH) {
		uint32_t v[BATCH];
#pragma unroll
		for (int u = 0; u < BATCH; u++) {
			const int it = tid + (u0 + u) * ROT_THREADS, xl = it & (T - 1), al = it / T;
			v[u] = 0;
			if (al < t.na && xl < t.nx) __builtin_memcpy(&v[u], r.in + rot_tile_in_row(r, t, al) + (size_t)xl * E, E);
		}
#pragma unroll
		for (int u = 0; u < BATCH; u++) {
			const int it = tid + (u0 + u) * ROT_THREADS, xl = it & (T - 1), al = it / T;
			if (al < t.na && xl < t.nx) lds[rot_lds_e(al, xl)] = v[u];
		}
	}
}
template <int E> DSP_HD void rot_tile_store_e(const RotArgs &r, const RotTile &t, const uint32_t *lds, int tid)
{
	constexpr int T = ROT_TILE_E;
	for (int it = tid; it < T * T; it += ROT_THREADS) {
		const int pos = it & (T - 1), xl = it / T;
		if (xl >= t.nx) break;
		if (pos >= t.na) continue;
		const uint32_t v = lds[rot_lds_e(rot_tile_a_of(r, t, pos), xl)];
		rot_store_n<E>(r.out + rot_tile_out_row(r, t, xl) + (size_t)pos * E, &v);
	}
}

}  // namespace dspfft
