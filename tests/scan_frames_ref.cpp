// TEST-ONLY: scan's frame loop (scan/scan.c:366-375, 379-417, 419-527) restated over scan_frame_core.h, the arithmetic the device kernels
// use.  Built with g++ -ffp-contract=off by tests/scan_frames_ref.py.  The scan order comes in as per-index coordinate lists (CSR); the
// inverse is either the stub of scan_frames_stub.h (what the reference-line fixtures are generated with) or, per frame, a given image
// (the device's own, to check the kernels bit for bit).
#include <stdint.h>
#include <string.h>
#include <vector>

#include "scan_frame_core.h"
extern "C" {
#include "scan_frames_stub.h"
}

using namespace dspfft;

extern "C" int sfr_run(uint32_t w, uint32_t h, const float *coeffs, const float *original, int depth, uint64_t limit, const uint64_t *off,
                       const uint32_t *yx, uint64_t step, uint64_t offset, uint64_t nframes, int invert, int fill, int visualize, int spectrogram,
                       int intermediates, int maxint, double gain, int scaletype, int signtype, const float *images, float *frames, uint64_t *parity)
{
	const size_t npix = (size_t)w * h, n = npix * 3;
	const size_t fw = (size_t)w * (1 + !!visualize), fh = (size_t)h * (1 + !!intermediates), ff = 3 * fw * fh;
	std::vector<float> frame(ff, 0.0f), sum(n), recon(n), image(n);
	const SfScaler sp = sf_scaler(scaletype, signtype, gain, coeffs[0], coeffs[1], coeffs[2]);
	auto set = [&](size_t x, size_t y, int z, float v) { frame[sf_frame_offset(fw, fh, x, y, z)] = v; };
	auto inverse = [&]() {
		if (images) { memcpy(image.data(), images, n * 4); images += n; }
		else sf_stub_redft01_2d(recon.data(), image.data(), w, h, 3);
	};
	for (size_t i = 0; i < npix; i++) memcpy(&sum[i * 3], coeffs, 12);
	if (fill) {
		std::fill(recon.begin(), recon.end(), 0.0f);
		for (uint64_t i = 0; i < offset; i++) {
			const uint64_t j = invert ? limit - i - 1 : i;
			for (uint64_t k = off[j]; k < off[j + 1]; k++) {
				const size_t y = yx[2 * k], x = yx[2 * k + 1], p = y * w + x;
				memcpy(&recon[p * 3], &coeffs[p * 3], 12);
				if (visualize)
					for (int z = 0; z < 3; z++) set(x + w, y, z, sf_mark_value(spectrogram, sp, coeffs[p * 3 + z], (uint32_t)x, (uint32_t)y));
			}
		}
		memset(recon.data(), 0, 12);
		inverse();
		for (size_t j = 0; j < n; j++) { SF_NO_CONTRACT sum[j] += image[j]; }
	}
	std::vector<size_t> lit;
	uint64_t par = ~0ull;
	for (uint64_t i = offset; i < offset + nframes; i++) {
		lit.clear();
		std::fill(recon.begin(), recon.end(), 0.0f);
		for (uint64_t s = i * step; s < i * step + step && s < limit; s++) {
			const uint64_t j = invert ? limit - s - 1 : s;
			for (uint64_t k = off[j]; k < off[j + 1]; k++) {
				const size_t y = yx[2 * k], x = yx[2 * k + 1], p = y * w + x;
				lit.push_back(p);
				memcpy(&recon[p * 3], &coeffs[p * 3], 12);
				if (visualize)
					for (int z = 0; z < 3; z++) {
						const float c = sf_mark_value(spectrogram, sp, coeffs[p * 3 + z], (uint32_t)x, (uint32_t)y);
						set(x + w, y, z, c);
						if (intermediates) set(x + w, y + h, z, c);
					}
			}
		}
		memset(recon.data(), 0, 12);
		inverse();
		for (size_t y = 0; y < h; y++)
			for (size_t x = 0; x < w; x++)
				for (int z = 0; z < 3; z++) {
					SF_NO_CONTRACT
					const size_t j = (y * w + x) * 3 + z;
					sum[j] += image[j];
					set(x, y, z, sum[j]);
				}
		if (intermediates) {
			float mn[3], mx[3];
			if (maxint) {
				for (int z = 0; z < 3; z++) mx[z] = mn[z] = image[z];
				for (size_t j = 1; j < npix; j++)
					for (int z = 0; z < 3; z++) {
						const float c = image[j * 3 + z];
						if (c > mx[z]) mx[z] = c;
						else if (c < mn[z]) mn[z] = c;
					}
				for (int z = 0; z < 3; z++) { SF_NO_CONTRACT mx[z] = mx[z] + coeffs[z]; mn[z] = mn[z] + coeffs[z]; }
			} else
				for (int z = 0; z < 3; z++) { mn[z] = 0; mx[z] = 1; }
			for (size_t y = 0; y < h; y++)
				for (size_t x = 0; x < w; x++)
					for (int z = 0; z < 3; z++) set(x, y + h, z, sf_intermediate(image[(y * w + x) * 3 + z], coeffs[z], mn[z], mx[z]));
		}
		memcpy(frames, frame.data(), ff * 4);
		frames += ff;
		if (intermediates && visualize)
			for (size_t p : lit)
				for (int z = 0; z < 3; z++) set(p % w + w, p / w + h, z, 0.0f);
		if (depth && par == ~0ull) {
			bool at = true;
			for (size_t j = 0; j < n && at; j++) at = !sf_parity_differs(original[j], sum[j], depth);
			if (at) par = i - offset;
		}
	}
	*parity = par;
	return 0;
}

// the top-right panel's value of every coefficient (HWC), with the gain rounded to float as spec_create rounds it (round_gain) or
// kept in double (what the reference does NOT do; tests/test_scan_frames_cpu.py shows the difference)
extern "C" void sfr_spec_values(uint32_t w, uint32_t h, const float *coeffs, double gain, int round_gain, int scaletype, int signtype, float *out)
{
	SfScaler s = sf_scaler(scaletype, signtype, gain, coeffs[0], coeffs[1], coeffs[2]);
	if (!round_gain) {
		SF_NO_CONTRACT
		float mx = coeffs[0];
		for (int z = 1; z < 3; z++) if (coeffs[z] > mx) mx = coeffs[z];
		s.gain = gain;
		s.max = sf_scale(scaletype, gain * (double)mx);
	}
	for (uint32_t y = 0; y < h; y++)
		for (uint32_t x = 0; x < w; x++)
			for (int z = 0; z < 3; z++) out[((size_t)y * w + x) * 3 + z] = sf_spec_value(s, coeffs[((size_t)y * w + x) * 3 + z], sf_normalization_2d(x, y));
}
