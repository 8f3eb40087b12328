// What api.cpp and multi_gpu.cpp share that include/skr.h does not declare.
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/skr.h"

void skr_set_error(const char *fmt, ...); // scene_host.cpp

#define SKR_HIP(call)                                                                                      \
	do                                                                                                     \
	{                                                                                                      \
		hipError_t e_ = (call);                                                                            \
		if(e_ != hipSuccess)                                                                               \
		{                                                                                                  \
			skr_set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__);     \
			return SKR_ERR_HIP;                                                                            \
		}                                                                                                  \
	} while(0)

// (api.cpp) a clone follows its source's development switches: tests change them between frames
void skr_copy_switches(skr_renderer *dst, const skr_renderer *src);
// (api.cpp) skr_render_tile_list for a table the caller owns and never rewrites in place: table_id (not 0) names its contents
int skr_render_tile_list_owned(skr_renderer *r, const skr_options *opt, uint32_t tile_rows, const uint32_t *d_tiles, uint32_t n_slots, uint64_t table_id, uint8_t *d_rgb,
							   float *d_rgbf, void *stream);
