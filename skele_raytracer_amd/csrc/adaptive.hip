// Adaptive sampling (include/skr.h skr_render_adaptive): the per-pixel statistics of a progressive render, the
// selection of the pixels that are still noisy, and the pieces of a round that gives only those pixels one more pass.
//
//   skr_adaptive_fold_kernel     a frame's pixels (all, or the listed ones, gathered) into the running sums C, S1, S2, n
//   skr_adaptive_count_kernel    } the still-active pixels of a list, compacted in ascending pixel order: per workgroup of 256
//   skr_adaptive_scan_kernel     } entries its survivors (wave ballots), one workgroup's exclusive scan of those counts, then the
//   skr_adaptive_scatter_kernel  } scatter (rank in the wave by mbcnt, the waves before it through LDS, the workgroup's offset)
//   skr_adaptive_rays_kernel     the camera rays of the listed pixels, bit for bit those of skr_camera_rays (primary_ray)
//   skr_adaptive_sample_kernel   one AA sample of the listed pixels' shading queries: summed in sample order, divided by g^2 after
//                                the last, then folded
//   skr_adaptive_resolve_kernel  the mean C / n, its bytes and n; skr_adaptive_resolve_var_kernel: and the variance of that mean
//
// Every list holds a pixel at most once, so each update is a plain read-modify-write of that pixel's state: no atomics, and the
// sums are formed in pass order whatever the schedule.  Plain streams of 24 bytes of state per listed pixel (HBM-bound).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "launch.h"
#include "skr.h"
#include "wave_common.h"

// pass k of pixel p: C += v, S1 += l, S2 += l * l, n += 1 (the first pass sets them)
SKR_DEV void adaptive_add(const AdaptiveScratch &s, uint32_t p, float r, float g, float b, bool first)
{
	const float l = sk_lum(r, g, b);
	const float l2 = l * l;
	if(first)
	{
		s.st[p] = make_float4(r, g, b, l);
		s.st2[p] = make_uint2(__float_as_uint(l2), 1u);
		return;
	}
	float4 c = s.st[p];
	const uint2 q = s.st2[p];
	c.x = c.x + r;
	c.y = c.y + g;
	c.z = c.z + b;
	c.w = c.w + l;
	s.st[p] = c;
	s.st2[p] = make_uint2(__float_as_uint(__uint_as_float(q.x) + l2), q.y + 1u);
}

// include/skr.h: does pixel p get pass n, n the passes it has had
SKR_DEV bool adaptive_active(const AdaptiveScratch &s, const AdaptiveRule &rule, uint32_t p)
{
	const uint32_t n = s.st2[p].y;
	if(n < rule.min_passes) return true;
	if(n >= rule.max_passes) return false;
	if(!(rule.threshold >= 0.0f) || n < 2) return true; // the test does not run: not converged
	const float nf = (float) n;
	const float m = sk_divf(s.st[p].w, nf);
	const float d = sk_divf(__uint_as_float(s.st2[p].x), nf) - m * m;
	const float var = d > 0.0f ? d : 0.0f;
	const float e2 = sk_divf(var, nf - 1.0f);
	const float b = rule.threshold * (m > SKR_ADAPTIVE_LUM_FLOOR ? m : SKR_ADAPTIVE_LUM_FLOOR);
	return !(e2 <= b * b);
}

__global__ __launch_bounds__(256) void skr_adaptive_fold_kernel(const AdaptiveScratch s, const float *__restrict__ frame, const uint32_t *__restrict__ list, uint32_t m,
																 int first)
{
	const size_t stride = (size_t) gridDim.x * 256;
	for(size_t i = (size_t) blockIdx.x * 256 + threadIdx.x; i < m; i += stride)
	{
		const size_t p = list ? list[i] : i;
		adaptive_add(s, (uint32_t) p, frame[3 * p], frame[3 * p + 1], frame[3 * p + 2], first != 0);
	}
}

__global__ __launch_bounds__(256) void skr_adaptive_count_kernel(const AdaptiveScratch s, const AdaptiveRule rule, const uint32_t *__restrict__ in, uint32_t m)
{
	__shared__ uint32_t wsum[4];
	const uint64_t i = (uint64_t) blockIdx.x * 256 + threadIdx.x;
	const bool keep = i < m && adaptive_active(s, rule, in ? in[i] : (uint32_t) i);
	const uint64_t bal = __ballot(keep);
	if((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = (uint32_t) __popcll(bal);
	__syncthreads();
	if(threadIdx.x == 0) s.blocks[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// one workgroup: blocks[j] = survivors of the workgroups before j; *count = all survivors
__global__ __launch_bounds__(256) void skr_adaptive_scan_kernel(uint32_t *__restrict__ blocks, uint32_t nb, uint32_t *__restrict__ count)
{
	__shared__ uint32_t wsum[4];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	uint32_t carry = 0;
	for(uint32_t base = 0; base < nb; base += 256)
	{
		const uint32_t j = base + threadIdx.x;
		const uint32_t v = j < nb ? blocks[j] : 0u;
		uint32_t x = v;
#pragma unroll
		for(int d = 1; d < 64; d <<= 1)
		{
			const uint32_t y = __shfl_up(x, d);
			if(lane >= d) x += y;
		}
		if(lane == 63) wsum[wave] = x;
		__syncthreads();
		uint32_t before = 0, total = 0;
#pragma unroll
		for(int w = 0; w < 4; w++)
		{
			before += w < wave ? wsum[w] : 0u;
			total += wsum[w];
		}
		if(j < nb) blocks[j] = carry + before + x - v;
		carry += total;
		__syncthreads(); // (wsum is rewritten by the next chunk)
	}
	if(threadIdx.x == 0) *count = carry;
}

__global__ __launch_bounds__(256) void skr_adaptive_scatter_kernel(const AdaptiveScratch s, const AdaptiveRule rule, const uint32_t *__restrict__ in, uint32_t m,
																	uint32_t *__restrict__ out)
{
	__shared__ uint32_t wsum[4];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const uint64_t i = (uint64_t) blockIdx.x * 256 + threadIdx.x;
	const uint32_t p = i < m ? (in ? in[i] : (uint32_t) i) : 0u;
	const bool keep = i < m && adaptive_active(s, rule, p);
	const uint64_t bal = __ballot(keep);
	const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t) (bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) bal, 0u));
	if(lane == 0) wsum[wave] = (uint32_t) __popcll(bal);
	__syncthreads();
	uint32_t off = s.blocks[blockIdx.x];
#pragma unroll
	for(int w = 0; w < 4; w++) off += w < wave ? wsum[w] : 0u;
	if(keep) out[off + rank] = p;
}

// skr_camera_ray_kernel (trace_rays.hip) for the pixels of a list: lane i writes the rays of pixel list[i] to slot i
__global__ __launch_bounds__(256) void skr_adaptive_rays_kernel(const RenderParams p, const uint32_t *__restrict__ list, uint32_t m, float4 *__restrict__ rays)
{
	const uint64_t i = (uint64_t) blockIdx.x * 256u + threadIdx.x;
	if(i >= m) return;
	const uint32_t pix = list[i], w = (uint32_t) p.width;
	const uint32_t y = pix / w, x = pix - y * w;
	f3 dir;
	primary_ray(p, (int) x, y, pix, p.aa_index, dir);
	rays[2 * i] = make_float4(p.cam_pos.x, p.cam_pos.y, p.cam_pos.z, __builtin_inff());
	rays[2 * i + 1] = make_float4(dir.x, dir.y, dir.z, __int_as_float(-1));
}

// The same under a lens (include/skr.h skr_scene_set_lens): (o', d') of wave_common.h lens_ray, the rays of skr_camera_ray_lens_kernel
__global__ __launch_bounds__(256) void skr_adaptive_rays_lens_kernel(const RenderParams p, const uint32_t *__restrict__ list, uint32_t m, float4 *__restrict__ rays, const Lens lens)
{
	const uint64_t i = (uint64_t) blockIdx.x * 256u + threadIdx.x;
	if(i >= m) return;
	const uint32_t pix = list[i], w = (uint32_t) p.width;
	const uint32_t y = pix / w, x = pix - y * w;
	f3 dir, o;
	primary_ray(p, (int) x, y, pix, p.aa_index, dir);
	lens_ray(p, lens, pix, p.aa_index, dir, o, dir);
	rays[2 * i] = make_float4(o.x, o.y, o.z, __builtin_inff());
	rays[2 * i + 1] = make_float4(dir.x, dir.y, dir.z, __int_as_float(-1));
}

// AA sample `a` of `samples` (0: one sample at the pixel centre, folded as it is) of the listed pixels, slot i = pixel list[i]:
// the running sum starts at 0 and adds the samples in sample order, then / (float) samples (render_wave.hip skr_resolve_kernel)
__global__ __launch_bounds__(256) void skr_adaptive_sample_kernel(const AdaptiveScratch s, const uint32_t *__restrict__ list, uint32_t m, uint32_t a, uint32_t samples)
{
	const size_t stride = (size_t) gridDim.x * 256;
	for(size_t i = (size_t) blockIdx.x * 256 + threadIdx.x; i < m; i += stride)
	{
		float r = s.shade[3 * i], g = s.shade[3 * i + 1], b = s.shade[3 * i + 2];
		if(samples > 0)
		{
			const bool first = a == 0;
			r = (first ? 0.0f : s.sacc[3 * i]) + r;
			g = (first ? 0.0f : s.sacc[3 * i + 1]) + g;
			b = (first ? 0.0f : s.sacc[3 * i + 2]) + b;
			if(a + 1 < samples)
			{
				s.sacc[3 * i] = r;
				s.sacc[3 * i + 1] = g;
				s.sacc[3 * i + 2] = b;
				continue;
			}
			const float d = (float) samples;
			r = sk_divf(r, d);
			g = sk_divf(g, d);
			b = sk_divf(b, d);
		}
		adaptive_add(s, list[i], r, g, b, false);
	}
}

// VAR: also var_p, the variance of the mean luminance (include/skr.h skr_render_adaptive_var): the e2 of adaptive_active, -1 under two passes
template <bool VAR>
SKR_DEV void adaptive_resolve(const AdaptiveScratch &s, uint64_t pixels, uint8_t *rgb, float *rgbf, uint32_t *passes, float *var)
{
	const size_t stride = (size_t) gridDim.x * 256;
	for(size_t p = (size_t) blockIdx.x * 256 + threadIdx.x; p < pixels; p += stride)
	{
		const float4 c = s.st[p];
		const uint32_t n = s.st2[p].y;
		const float nf = (float) n;
		const float r = sk_divf(c.x, nf), g = sk_divf(c.y, nf), b = sk_divf(c.z, nf);
		if(rgbf)
		{
			rgbf[3 * p] = r;
			rgbf[3 * p + 1] = g;
			rgbf[3 * p + 2] = b;
		}
		if(rgb)
		{
			rgb[3 * p] = (uint8_t) quantise(r);
			rgb[3 * p + 1] = (uint8_t) quantise(g);
			rgb[3 * p + 2] = (uint8_t) quantise(b);
		}
		if(passes) passes[p] = n;
		if constexpr(VAR)
		{
			float v = -1.0f; // not measured
			if(n >= 2)
			{
				const float m = sk_divf(c.w, nf);
				const float d = sk_divf(__uint_as_float(s.st2[p].x), nf) - m * m;
				v = sk_divf(d > 0.0f ? d : 0.0f, nf - 1.0f);
			}
			var[p] = v;
		}
	}
}

__global__ __launch_bounds__(256) void skr_adaptive_resolve_kernel(const AdaptiveScratch s, uint64_t pixels, uint8_t *__restrict__ rgb, float *__restrict__ rgbf,
																	uint32_t *__restrict__ passes)
{
	adaptive_resolve<false>(s, pixels, rgb, rgbf, passes, nullptr);
}

// the same, and var_p of every pixel (one more 4-byte store)
__global__ __launch_bounds__(256) void skr_adaptive_resolve_var_kernel(const AdaptiveScratch s, uint64_t pixels, uint8_t *__restrict__ rgb, float *__restrict__ rgbf,
																		uint32_t *__restrict__ passes, float *__restrict__ var)
{
	adaptive_resolve<true>(s, pixels, rgb, rgbf, passes, var);
}

static unsigned stream_blocks(uint64_t n)
{
	const uint64_t b = (n + 255) / 256;
	return (unsigned) (b < 1 ? 1 : b > 4096 ? 4096 : b); // grid-stride: 16 workgroups per CU keep HBM busy (accumulate.hip)
}

static size_t align256(size_t x) { return (x + 255) & ~(size_t) 255; }

// one allocation: st | st2 | list 0 | list 1 | blocks + count | rays | shade | sacc, each part 256-byte aligned (92 bytes a pixel)
static AdaptiveScratch carve(char *base, uint64_t pixels, size_t &total)
{
	const size_t n = (size_t) pixels, nb = (n + 255) / 256;
	AdaptiveScratch s{};
	size_t o = 0;
	auto take = [&](size_t bytes) { char *q = base ? base + o : nullptr; o += align256(bytes); return q; };
	s.st = reinterpret_cast<float4 *>(take(n * sizeof(float4)));
	s.st2 = reinterpret_cast<uint2 *>(take(n * sizeof(uint2)));
	s.list[0] = reinterpret_cast<uint32_t *>(take(n * sizeof(uint32_t)));
	s.list[1] = reinterpret_cast<uint32_t *>(take(n * sizeof(uint32_t)));
	s.blocks = reinterpret_cast<uint32_t *>(take((nb + 1) * sizeof(uint32_t)));
	s.count = s.blocks ? s.blocks + nb : nullptr;
	s.rays = reinterpret_cast<float4 *>(take(n * 2 * sizeof(float4)));
	s.shade = reinterpret_cast<float *>(take(n * 3 * sizeof(float)));
	s.sacc = reinterpret_cast<float *>(take(n * 3 * sizeof(float)));
	total = o;
	return s;
}

size_t skr_adaptive_scratch_bytes(uint64_t pixels)
{
	size_t total = 0;
	(void) carve(nullptr, pixels, total);
	return total;
}

AdaptiveScratch skr_adaptive_carve(void *base, uint64_t pixels)
{
	size_t total = 0;
	return carve(static_cast<char *>(base), pixels, total);
}

hipError_t skr_launch_adaptive_fold(const AdaptiveScratch &s, const float *frame, const uint32_t *list, uint32_t m, int first, hipStream_t stream)
{
	if(m == 0) return hipSuccess;
	hipLaunchKernelGGL(skr_adaptive_fold_kernel, dim3(stream_blocks(m)), dim3(256), 0, stream, s, frame, list, m, first);
	return hipGetLastError();
}

hipError_t skr_launch_adaptive_select(const AdaptiveScratch &s, const AdaptiveRule &rule, const uint32_t *in, uint32_t m, uint32_t *out, hipStream_t stream)
{
	if(m == 0) return hipMemsetAsync(s.count, 0, sizeof(uint32_t), stream);
	const uint32_t nb = (uint32_t) (((uint64_t) m + 255) / 256);
	hipLaunchKernelGGL(skr_adaptive_count_kernel, dim3(nb), dim3(256), 0, stream, s, rule, in, m);
	hipLaunchKernelGGL(skr_adaptive_scan_kernel, dim3(1), dim3(256), 0, stream, s.blocks, nb, s.count);
	hipLaunchKernelGGL(skr_adaptive_scatter_kernel, dim3(nb), dim3(256), 0, stream, s, rule, in, m, out);
	return hipGetLastError();
}

hipError_t skr_launch_adaptive_rays(const RenderParams &p, const uint32_t *list, uint32_t m, float4 *rays, hipStream_t stream, const Lens *lens)
{
	if(m == 0) return hipSuccess;
	if(lens) hipLaunchKernelGGL(skr_adaptive_rays_lens_kernel, dim3((unsigned) (((uint64_t) m + 255) / 256)), dim3(256), 0, stream, p, list, m, rays, *lens);
	else hipLaunchKernelGGL(skr_adaptive_rays_kernel, dim3((unsigned) (((uint64_t) m + 255) / 256)), dim3(256), 0, stream, p, list, m, rays);
	return hipGetLastError();
}

hipError_t skr_launch_adaptive_sample(const AdaptiveScratch &s, const uint32_t *list, uint32_t m, uint32_t sample, uint32_t samples, hipStream_t stream)
{
	if(m == 0) return hipSuccess;
	hipLaunchKernelGGL(skr_adaptive_sample_kernel, dim3(stream_blocks(m)), dim3(256), 0, stream, s, list, m, sample, samples);
	return hipGetLastError();
}

hipError_t skr_launch_adaptive_resolve(const AdaptiveScratch &s, uint64_t pixels, uint8_t *rgb, float *rgbf, uint32_t *passes, float *var, hipStream_t stream)
{
	if(pixels == 0) return hipSuccess;
	if(var) hipLaunchKernelGGL(skr_adaptive_resolve_var_kernel, dim3(stream_blocks(pixels)), dim3(256), 0, stream, s, pixels, rgb, rgbf, passes, var);
	else hipLaunchKernelGGL(skr_adaptive_resolve_kernel, dim3(stream_blocks(pixels)), dim3(256), 0, stream, s, pixels, rgb, rgbf, passes);
	return hipGetLastError();
}
