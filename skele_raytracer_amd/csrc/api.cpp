// C ABI glue: device context, scene upload, launches (include/skr.h).
// There is deliberately no CPU fallback: without a usable HIP device every
// device entry point fails with SKR_ERR_NO_DEVICE / SKR_ERR_HIP.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <vector>

#include "api_internal.h"
#include "launch.h"
#include "scene_pack.h"

static thread_local const char *g_variant = "none";

// The counter block of a scene (DeviceScene::d_counters), in 64-bit words: the work counters, SKR_COUNTER_SHARDS x {radiance rays,
// sphere hits shaded, shadow rays, sphere tests}; the 8 phase stamps of diagnostic builds (wave_common.h); then the queue counters,
// 32-bit words SKR_PULL_STRIDE apart, and 8 reserved words behind them.  The walks' counters are allocations of their own.
constexpr size_t CTR_WORK_WORDS = (size_t) SKR_COUNTER_SHARDS * 4, CTR_STAMP_WORDS = 8, CTR_RESERVED_WORDS = 8;
constexpr size_t CTR_READ_WORDS = CTR_WORK_WORDS + CTR_STAMP_WORDS; // what the readers copy and reset, and where the queue counters start
constexpr size_t CTR_BYTES = (CTR_READ_WORDS + CTR_RESERVED_WORDS) * sizeof(unsigned long long) + (SKR_PULL_QUEUES + 2 + 2 * SKR_P1_REGIONS) * SKR_PULL_STRIDE * sizeof(uint32_t);
constexpr size_t CTR_SNAP_BYTES = 2 * CTR_WORK_WORDS * sizeof(unsigned long long); // skr_renderer::d_snap: the work counters twice (render_params.h SkrTimingHook)
constexpr size_t WALK_SHARDS = 256; // d_tri_work, d_st_work: WALK_SHARDS x {culling-sphere tests, leaf tests} of a walk
constexpr size_t WALK_BYTES = WALK_SHARDS * 2 * sizeof(unsigned long long);

// The uploaded scene: shared by a renderer and its clones (skr_renderer_clone), freed by the last of them.  Every pointer is null or
// came from hipMalloc.
struct DeviceScene {
	int device = 0;
	int lds_limit = 0;
	skr_scene_info info{};
	SceneLayout layout; // where the sections of d_blob lie (scene_pack.h)
	float4 *d_blob = nullptr;
	float4 *d_camec = nullptr; // per sphere {cam_pos - centre, |.|^2 - r^2} (render_wave.hip skr_camec_kernel), + SKR_BLOB_PAD_ROWS rows of padding
	unsigned long long *d_counters = nullptr; // CTR_BYTES
	unsigned long long *d_tri_work = nullptr; // the triangle walks' counters (skr_renderer_read_triangle_work)
	unsigned long long *d_st_work = nullptr;  // the sphere tree's (skr_renderer_read_sphere_tree_work); null without a sphere tree
	float4 *d_vel = nullptr; // the spheres' velocities {v.xyz, 0} in file order, + SKR_BLOB_PAD_ROWS rows of zeros (launch.h Motion); null unless motion is in force

	float4 *d_env = nullptr; // the environment's texels {r, g, b, 0}, edge * edge rows, row j first (launch.h EnvMap); null unless the scene has an environment

	float4 *d_tex = nullptr; // the textures: one row pair {texel offset, edge} per sphere in file order (edge 0: none), padded to whole 16-byte rows, then every texture's texels
	                         // {r, g, b, 0}, row j first (launch.h Textures); null unless textures are in force
	size_t tex_rows = 0;     // the float4 rows the per-sphere pairs take: the texels start behind them

	float4 *d_emit = nullptr; // the spheres' emission {r, g, b, 0} in file order (launch.h Emission); null unless emission is in force.  With it d_tex exists too, every edge 0
	                          // where the scene has no texture: a launch with emission carries Textures (render_generic.hip with_pack)

	DeviceScene() = default;
	DeviceScene(const DeviceScene &) = delete;
	DeviceScene &operator=(const DeviceScene &) = delete;
	~DeviceScene()
	{
		for(void *p : {(void *) d_blob, (void *) d_camec, (void *) d_counters, (void *) d_tri_work, (void *) d_st_work, (void *) d_vel, (void *) d_env, (void *) d_tex, (void *) d_emit})
			if(p) (void) hipFree(p);
	}
};

// A device buffer grown on demand and kept.  grow() frees the old buffer first (hipFree waits for the launches that may still read
// it), then allocates exactly `need` bytes.
struct Scratch {
	void *p = nullptr;
	size_t bytes = 0;

	int grow(size_t need)
	{
		if(need <= bytes) return SKR_OK;
		if(p) SKR_HIP(hipFree(p));
		p = nullptr;
		bytes = 0;
		SKR_HIP(hipMalloc(&p, need));
		bytes = need;
		return SKR_OK;
	}
	template <class T> T *at(size_t off) const { return reinterpret_cast<T *>(static_cast<char *>(p) + off); }
	Scratch() = default;
	Scratch(const Scratch &) = delete;
	Scratch &operator=(const Scratch &) = delete;
	~Scratch() { if(p) (void) hipFree(p); }
};

struct skr_renderer {
	std::shared_ptr<const DeviceScene> scene;
	SkrSwitches sw; // the SKR_* development switches, read once (load_switches)
	// scratch (Scratch)
	Scratch nodes;   // level pipelines: every table of one band (launch.h NodePlan, GPlan)
	Scratch acc;     // their AA accumulation image (LaunchPlan::acc_bytes)
	Scratch prog;    // progressive accumulation: this pass's float frame | the running sum (progressive_scratch)
	Scratch frame;   // the *_host entries' device frame (host_frame)
	Scratch dn;      // skr_denoise(_var): the ping-pong images, the guides and the classes (launch.h DenoiseScratch)
	Scratch dnframe; // skr_render_denoised_host, skr_render_adaptive_denoised_host: the frame (and its variance and passes), its camera rays and guides, the filtered frame and its bytes
	Scratch ad;      // skr_render_adaptive: the per-pixel statistics, the active lists and the query path's rays (launch.h AdaptiveScratch)
	unsigned long long *d_snap = nullptr; // skr_renderer_kernel_work: the work counters in front of and behind the dominant kernel of the last timed launch
	uint32_t *h_count = nullptr; // skr_render_adaptive: the pinned word each round's active count is read back into
	hipEvent_t frame_e0 = nullptr, frame_e1 = nullptr; // the *_host entries' timing (timed_host)
	size_t last_off_ctr = 0; // the node-pipeline counters of the launch last enqueued (skr_renderer_last_*_count): where in `nodes` ...
	int last_levels = 0;     // ... and how many levels they count (0: the launch took another path)
	int last_leaf_shape = -1; // skr_renderer_last_leaf_shape
	int last_leaf_pow = -1;   // skr_renderer_last_leaf_pow
	bool timing = false;
	bool count_tri = false; // skr_renderer_count_triangle_work
	// the node pipeline's level-0 stage kept in `nodes` (launch.h PrimaryKey, take_node_scratch)
	PrimaryKey level0_key{};
	bool level0_kept = false;
	uint64_t level0_builds = 0, level0_replays = 0; // skr_renderer_primary_cache_stats
	// skr_renderer_kernel_ms: event pairs around the dominant kernel of recent launches
	std::vector<SkrTimingHook> timed;
	std::vector<SkrTimingHook> free_pairs;
};

// The level pipelines' scratch of `need` bytes, for a launch that will overwrite it.  Whoever takes `nodes` takes it here: the level-0
// stage a node-pipeline frame may have left in it (launch.h PrimaryKey) is forgotten, and only render_pass, which knows what it
// launches, keeps one again.  *kept: the stage was still there, in an allocation that did not move.
static int take_node_scratch(skr_renderer *r, size_t need, bool *kept = nullptr)
{
	const size_t had = r->nodes.bytes;
	const bool was_kept = r->level0_kept;
	r->level0_kept = false;
	const int rc = r->nodes.grow(need);
	if(kept) *kept = rc == SKR_OK && was_kept && r->nodes.bytes == had;
	return rc;
}

static void load_switches(SkrSwitches &sw)
{
	sw = SkrSwitches();
	if(const char *e = getenv("SKR_PIPELINE"))
		sw.pipeline = !strcmp(e, "nodes") ? SKR_PIPE_NODES : !strcmp(e, "generic") ? SKR_PIPE_GENERIC : SKR_PIPE_OTHER;
	sw.no_cones = getenv("SKR_NO_CONES") != nullptr;
	sw.no_cull = getenv("SKR_NO_CULL") != nullptr;
	if(const char *e = getenv("SKR_NO_SPHERE_CULL")) sw.no_sphere_cull = atoi(e) > 0 ? 1 : 0;
	if(const char *e = getenv("SKR_LEVELS_BUDGET_MB")) sw.budget_mb = atoi(e) > 0 ? atoi(e) : 1;
	if(const char *e = getenv("SKR_FLAT")) sw.flat = atoi(e) > 0 ? 1 : -1;
	if(const char *e = getenv("SKR_SHADOW_MASK")) sw.shadow_mask = (sw.shadow_mask & ~1) | (atoi(e) > 0 ? 1 : 0);
	if(const char *e = getenv("SKR_GI_MASK")) sw.gi_mask = atoi(e) > 0 ? 1 : 0;
	if(const char *e = getenv("SKR_GI_SURFACE")) sw.gi_surface = atoi(e) > 0 ? 1 : 0;
	if(const char *e = getenv("SKR_SHADOW_SURFACE")) sw.shadow_mask = (sw.shadow_mask & ~2) | (atoi(e) > 0 ? 2 : 0);
	if(const char *e = getenv("SKR_LEAF_SHAPE")) sw.shadow_mask = (sw.shadow_mask & ~SKR_SW_LEAF_SHAPE) | (atoi(e) > 0 ? SKR_SW_LEAF_SHAPE : 0);
	if(const char *e = getenv("SKR_LEAF_POW")) sw.shadow_mask = (sw.shadow_mask & ~SKR_SW_LEAF_POW) | (atoi(e) > 0 ? SKR_SW_LEAF_POW : 0);
	if(const char *e = getenv("SKR_PRIMARY_CACHE")) sw.primary_cache = atoi(e) > 0 ? 1 : 0;
	if(const char *e = getenv("SKR_ADAPTIVE_PATH")) sw.adaptive_path = !strcmp(e, "frame") ? 1 : !strcmp(e, "query") ? 2 : 0;
}

void skr_copy_switches(skr_renderer *dst, const skr_renderer *src) { dst->sw = src->sw; }

// The device frame of a *_host entry, kept in the renderer: its bytes, its floats and, with `passes`, the adaptive sampler's pass counts
struct HostFrame {
	uint8_t *rgb;
	float *rgbf;
	uint32_t *passes;
};
static int host_frame(skr_renderer *r, size_t pixels, bool passes, HostFrame &f)
{
	ScratchLayout L;
	const size_t o_rgb = L.take(pixels * 3), o_rgbf = L.take(pixels * 12), o_passes = passes ? L.take(pixels * 4) : 0;
	const int rc = r->frame.grow(L.off);
	if(rc != SKR_OK) return rc;
	f = {r->frame.at<uint8_t>(o_rgb), r->frame.at<float>(o_rgbf), passes ? r->frame.at<uint32_t>(o_passes) : nullptr};
	return SKR_OK;
}

// A *_host entry's device work on the null stream, timed by the renderer's event pair: `run` enqueues it, then every output with a
// host array is copied back, and the elapsed milliseconds go to *ms (if not null).
struct HostCopy {
	void *host; // null: not wanted
	const void *device;
	size_t bytes;
};
template <class Run>
static int timed_host(skr_renderer *r, Run run, std::initializer_list<HostCopy> copies, float *ms)
{
	if(!r->frame_e0) SKR_HIP(hipEventCreate(&r->frame_e0));
	if(!r->frame_e1) SKR_HIP(hipEventCreate(&r->frame_e1));
	SKR_HIP(hipEventRecord(r->frame_e0, nullptr));
	const int rc = run();
	if(rc != SKR_OK) return rc;
	SKR_HIP(hipEventRecord(r->frame_e1, nullptr));
	for(const HostCopy &c : copies)
		if(c.host) SKR_HIP(hipMemcpy(c.host, c.device, c.bytes, hipMemcpyDeviceToHost));
	float t = 0;
	SKR_HIP(hipEventSynchronize(r->frame_e1));
	SKR_HIP(hipEventElapsedTime(&t, r->frame_e0, r->frame_e1));
	if(ms) *ms = t;
	return SKR_OK;
}

extern "C" {

int skr_device_count(void)
{
	int n = 0;
	if(hipGetDeviceCount(&n) != hipSuccess) return 0;
	return n;
}

int skr_renderer_create(const skr_scene *scene, int device, skr_renderer **out)
{
	if(!scene || !out)
	{
		skr_set_error("skr_renderer_create: null argument");
		return SKR_ERR_ARG;
	}
	*out = nullptr;
	int n = 0;
	if(hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n)
	{
		skr_set_error("no usable HIP device (count=%d, asked for %d); libskr has no CPU fallback", n, device);
		return SKR_ERR_NO_DEVICE;
	}
	SKR_HIP(hipSetDevice(device));
	hipDeviceProp_t prop;
	SKR_HIP(hipGetDeviceProperties(&prop, device));
	if(strncmp(prop.gcnArchName, "gfx950", 6) != 0)
	{
		skr_set_error("device %d is %s; libskr is built for gfx950 (MI355X) only", device, prop.gcnArchName);
		return SKR_ERR_NO_DEVICE;
	}
	if(scene->raw_fog.size() / 9 > SKR_FOG_MAX_VOLUMES)
	{
		skr_set_error("scene has %zu fog volumes; at most %d are supported", scene->raw_fog.size() / 9, SKR_FOG_MAX_VOLUMES);
		return SKR_ERR_UNSUPPORTED;
	}
	if(scene->n_spot() > SKR_SPOT_MAX_LIGHTS)
	{
		skr_set_error("scene has %d spot lights; at most %d are supported", scene->n_spot(), SKR_SPOT_MAX_LIGHTS);
		return SKR_ERR_UNSUPPORTED;
	}
	auto s = std::make_shared<DeviceScene>(); // (frees what was allocated if the upload fails)
	s->device = device;
	s->info = scene->info;
	s->lds_limit = (int) prop.sharedMemPerBlock;
	const std::vector<skr_f4> blob = skr_pack_scene(*scene, s->layout);
	const size_t ns = scene->sph_geom.size(), camec_bytes = (ns + SKR_BLOB_PAD_ROWS) * 16;
	auto zeroed = [](auto **p, size_t bytes) { // a device allocation of zeros
		const hipError_t e = hipMalloc((void **) p, bytes);
		return e == hipSuccess ? hipMemset(*p, 0, bytes) : e;
	};
	hipError_t e = hipMalloc((void **) &s->d_blob, blob.size() * 16);
	if(e == hipSuccess) e = hipMemcpy(s->d_blob, blob.data(), blob.size() * 16, hipMemcpyHostToDevice);
	if(e == hipSuccess) e = zeroed(&s->d_counters, CTR_BYTES);
	if(e == hipSuccess) e = zeroed(&s->d_tri_work, WALK_BYTES);
	if(e == hipSuccess && s->layout.sphere_tree) e = zeroed(&s->d_st_work, WALK_BYTES);
	if(e == hipSuccess) e = zeroed(&s->d_camec, camec_bytes);
	if(e == hipSuccess && s->layout.motion)
	{ // the velocities travel beside the blob, whose section table they are no part of (scene_pack.h)
		std::vector<skr_f4> vel(ns + SKR_BLOB_PAD_ROWS, skr_f4{0.0f, 0.0f, 0.0f, 0.0f});
		for(size_t i = 0; i < ns && 3 * i + 2 < scene->velocities.size(); i++) vel[i] = skr_f4{scene->velocities[3 * i], scene->velocities[3 * i + 1], scene->velocities[3 * i + 2], 0.0f};
		e = hipMalloc((void **) &s->d_vel, vel.size() * 16);
		if(e == hipSuccess) e = hipMemcpy(s->d_vel, vel.data(), vel.size() * 16, hipMemcpyHostToDevice);
	}
	if(e == hipSuccess && s->layout.env_edge > 0)
	{ // the environment travels beside the blob too: one allocation per device scene, shared by its clones
		const size_t n = (size_t) s->layout.env_edge * (size_t) s->layout.env_edge;
		std::vector<skr_f4> tex(n);
		for(size_t i = 0; i < n; i++) tex[i] = skr_f4{scene->env_texels[3 * i], scene->env_texels[3 * i + 1], scene->env_texels[3 * i + 2], 0.0f};
		e = hipMalloc((void **) &s->d_env, n * 16);
		if(e == hipSuccess) e = hipMemcpy(s->d_env, tex.data(), n * 16, hipMemcpyHostToDevice);
	}
	if(e == hipSuccess && (s->layout.textured || s->layout.emissive))
	{ // so do the textures: the per-sphere rows, then the texels of every texture some sphere names (emission alone: the rows, every edge 0)
		s->tex_rows = (ns * 8 + 15) / 16;
		std::vector<skr_f4> tex(s->tex_rows, skr_f4{0.0f, 0.0f, 0.0f, 0.0f});
		std::vector<uint32_t> first(scene->textures.size(), 0xFFFFFFFFu); // where texture k's texels start, once some sphere names it
		std::vector<uint32_t> pairs(s->tex_rows * 4, 0u);
		for(size_t i = 0; i < ns && i < scene->sphere_textures.size(); i++)
		{
			const int32_t k = scene->sphere_textures[i];
			if(k < 0 || (size_t) k >= scene->textures.size()) continue;
			const size_t E = (size_t) scene->texture_edges[(size_t) k];
			if(first[(size_t) k] == 0xFFFFFFFFu)
			{
				first[(size_t) k] = (uint32_t) (tex.size() - s->tex_rows);
				const std::vector<float> &t = scene->textures[(size_t) k];
				for(size_t j = 0; j < E * E; j++) tex.push_back(skr_f4{t[3 * j], t[3 * j + 1], t[3 * j + 2], 0.0f});
			}
			pairs[2 * i] = first[(size_t) k];
			pairs[2 * i + 1] = (uint32_t) E;
		}
		memcpy(tex.data(), pairs.data(), s->tex_rows * 16);
		e = hipMalloc((void **) &s->d_tex, tex.size() * 16);
		if(e == hipSuccess) e = hipMemcpy(s->d_tex, tex.data(), tex.size() * 16, hipMemcpyHostToDevice);
	}
	if(e == hipSuccess && s->layout.emissive)
	{ // and the emission: one row per sphere
		std::vector<skr_f4> emi(ns > 0 ? ns : 1, skr_f4{0.0f, 0.0f, 0.0f, 0.0f});
		for(size_t i = 0; i < ns && 3 * i + 2 < scene->emission.size(); i++) emi[i] = skr_f4{scene->emission[3 * i], scene->emission[3 * i + 1], scene->emission[3 * i + 2], 0.0f};
		e = hipMalloc((void **) &s->d_emit, emi.size() * 16);
		if(e == hipSuccess) e = hipMemcpy(s->d_emit, emi.data(), emi.size() * 16, hipMemcpyHostToDevice);
	}
	if(e == hipSuccess)
	{ // the camera belongs to the scene: its (e, c) rows are formed once, on the device, by the operations every ray would perform
		const float *c = scene->info.camera;
		e = skr_launch_camec(s->d_blob, (int) ns, f3{c[0], c[1], c[2]}, s->d_camec, nullptr);
		if(e == hipSuccess) e = hipDeviceSynchronize();
	}
	if(e != hipSuccess)
	{
		skr_set_error("scene upload failed: %s", hipGetErrorString(e));
		return SKR_ERR_HIP;
	}
	skr_renderer *r = new skr_renderer();
	r->scene = std::move(s);
	load_switches(r->sw);
	*out = r;
	return SKR_OK;
}

// A second renderer for the same scene on the same device with its own scratch (tables, accumulation buffers, timing events) — what a
// second frame in flight needs (multi_gpu.cpp: consecutive frames of a run alternate between a renderer and its clone on two streams).
// The scene blob (read-only) and the work counters (atomics) are SHARED with `src` (DeviceScene): rays counted by either are read
// through either.
int skr_renderer_clone(const skr_renderer *src, skr_renderer **out)
{
	if(!src || !out)
	{
		skr_set_error("skr_renderer_clone: null argument");
		return SKR_ERR_ARG;
	}
	*out = nullptr;
	SKR_HIP(hipSetDevice(src->scene->device));
	skr_renderer *r = new skr_renderer();
	r->scene = src->scene;
	r->sw = src->sw;
	*out = r;
	return SKR_OK;
}

void skr_renderer_destroy(skr_renderer *r)
{
	if(!r) return;
	(void) hipSetDevice(r->scene->device);
	if(r->d_snap) (void) hipFree(r->d_snap);
	if(r->h_count) (void) hipHostFree(r->h_count);
	if(r->frame_e0) (void) hipEventDestroy(r->frame_e0);
	if(r->frame_e1) (void) hipEventDestroy(r->frame_e1);
	for(SkrTimingHook &h : r->timed) { (void) hipEventDestroy(h.start); (void) hipEventDestroy(h.stop); }
	for(SkrTimingHook &h : r->free_pairs) { (void) hipEventDestroy(h.start); (void) hipEventDestroy(h.stop); }
	delete r; // (the scratch, and the scene with the last renderer that holds it)
}

uint32_t skr_tile_count(const skr_options *opt, uint32_t tile_rows, uint32_t first_tile, uint32_t tile_stride)
{
	if(!opt || opt->height <= 0 || tile_rows == 0 || tile_stride == 0) return 0;
	const uint32_t total = ((uint32_t) opt->height + tile_rows - 1) / tile_rows;
	if(first_tile >= total) return 0;
	return (total - first_tile + tile_stride - 1) / tile_stride;
}

static int check_options(const skr_options *opt)
{
	if(opt->width <= 0 || opt->height <= 0 || opt->width > 65536 || opt->height > 65536)
	{
		skr_set_error("bad image size %dx%d", opt->width, opt->height);
		return SKR_ERR_ARG;
	}
	if(opt->max_depth <= 0)
	{ // main.cpp:318-329: "depth takes a positive int"
		skr_set_error("depth takes a positive int after flag for the max depth");
		return SKR_ERR_ARG;
	}
	if(opt->grid_size < 0 || opt->grid_size > 1024 || opt->num_path_traces < 0 || opt->num_path_traces > 32767)
	{
		skr_set_error("jsample/gillum out of range (%d, %d)", opt->grid_size, opt->num_path_traces);
		return SKR_ERR_ARG;
	}
	return SKR_OK;
}

// What every launch starts from, and all the camera rays need (skr_launch_camera_rays, skr_launch_adaptive_rays): the size of the frame
// of opt, AA sample `sample` of it under `seed`, and the camera of camera.h:8-32 (what primary_ray() reads) with main.cpp:134-137
// hoisted (identical float/double expressions evaluated once)
static RenderParams camera_params(const skr_scene_info &info, const skr_options *opt, uint64_t seed, uint32_t sample)
{
	RenderParams p{};
	p.width = opt->width;
	p.height = opt->height;
	p.grid_size = opt->grid_size;
	p.seed_lo = (uint32_t) seed;
	p.seed_hi = (uint32_t) (seed >> 32);
	p.aa_index = sample;
	p.inv_width = 1 / float(opt->width);
	p.inv_height = 1 / float(opt->height);
	p.aspect = opt->width / float(opt->height);
	p.angle = (float) tan(M_PI * 0.5 * opt->fov / 180.);
	const float *c = info.camera;
	p.cam_pos = f3{c[0], c[1], c[2]};
	p.cam_dir = f3{c[3], c[4], c[5]};
	p.cam_up = f3{c[6], c[7], c[8]};
	p.cam_right = f3{c[9], c[10], c[11]};
	return p;
}

// one frame (one pass of a progressive render) of the tiles first_tile, first_tile + tile_stride, ...
// the tiles of a launch: first, first + stride, ... (table == nullptr) or the n_slots entries of a device table (skr_render_tile_list)
struct TileSel {
	uint32_t first = 0, stride = 1, max_tiles = 0xffffffffu;
	const uint32_t *d_table = nullptr;
	uint32_t n_slots = 0;
	uint64_t table_id = 0; // what the owner of d_table calls its present contents (skr_render_tile_list_owned); 0: the caller's memory, contents unknown
};
static uint32_t sel_tiles(const skr_options *opt, uint32_t tile_rows, const TileSel &ts)
{
	if(ts.d_table) return ts.n_slots;
	const uint32_t n = skr_tile_count(opt, tile_rows, ts.first, ts.stride);
	return n > ts.max_tiles ? ts.max_tiles : n;
}

// What the launch helpers below read of a renderer, and all they read: the scene's facts and layout, where its tables start, the
// switches and whether the walks count their work.  It owns nothing: a renderer's addresses are its DeviceScene's allocations,
// skr_scene_leaf_shape's are host arrays nobody dereferences.
struct LaunchScene {
	const skr_scene_info &info;
	const SceneLayout &layout;
	const float4 *blob, *camec;
	unsigned long long *counters, *tri_work, *st_work;
	const SkrSwitches &sw;
	bool count_tri;
	const float4 *vel; // the velocity rows where motion is in force (DeviceScene::d_vel)
	const float4 *env; // the environment's texels where the scene has one (DeviceScene::d_env)
	const float4 *tex; // the textures' rows and texels where textures are in force (DeviceScene::d_tex) ...
	size_t tex_rows;   // ... and how many rows the per-sphere pairs take
	const float4 *emit; // the emission rows where emission is in force (DeviceScene::d_emit)
	const float4 *sec(SkrBlobSection k) const { return blob + layout.first[k]; } // where a section starts
};
static LaunchScene launch_scene(const skr_renderer *r)
{
	const DeviceScene &s = *r->scene;
	return {s.info, s.layout, s.d_blob, s.d_camec, s.d_counters, s.d_tri_work, s.d_st_work, r->sw, r->count_tri, s.d_vel, s.d_env, s.d_tex, s.tex_rows, s.d_emit};
}
static float4 ball4(const skr_f4 &b) { return make_float4(b.x, b.y, b.z, b.w); }

// Everything of a launch beyond camera_params that is not its output: the scene, the switches and masks, and the options folded and
// checked — the depth fold, the node-id bound, the fog exclusions.  render_pass and skr_shade_rays both take it.
// query: a shading query — its rays are the caller's, so the scene's lens is not among its features.
static GenericFeatures generic_features(const LaunchScene &v, const RenderParams &p, bool query);
static int launch_params(const LaunchScene &v, const skr_options *opt, RenderParams &p, GenericFeatures &f, bool query = false)
{
	const SceneLayout &s = v.layout;
	p.sw = v.sw;
	const float *c = v.info.camera;
	p.background = f3{v.info.background[0], v.info.background[1], v.info.background[2]};
	p.n_spheres = v.info.n_spheres;
	p.n_tris = v.info.n_triangles;
	p.n_lights = v.info.n_point_lights + s.n_spot + v.info.n_directional_lights; // (spot lights only under --scn-spot, directional ones only under --strict-scn)
	p.sph_geom = v.blob;
	p.cam_ec = v.camec;
	p.sph_amb = v.sec(SKR_SEC_amb);
	p.sph_kd = v.sec(SKR_SEC_kd);
	p.sph_ks = v.sec(SKR_SEC_ks);
	p.lights = v.sec(SKR_SEC_lights);
	p.tris = v.sec(SKR_SEC_tris);
	p.tri_chunks = v.sec(SKR_SEC_chunks);
	p.tri_chunk_size = s.chunk_size;
	p.tri_cones = (s.cones && !v.sw.no_cones) ? 1 : 0;
	if(s.has(SKR_SEC_smask) && (v.sw.shadow_mask & 1))
	{ // the level pipelines' shadow walk visits only the spheres a lane's masks name (shade_common.h occluded_pair)
		p.shadow_masks = reinterpret_cast<const uint32_t *>(v.sec(SKR_SEC_smask));
		p.shadow_reach2 = s.shadow_reach2;
		p.shadow_all = p.n_spheres >= 32 ? ~0u : (1u << p.n_spheres) - 1u;
		if(s.has(SKR_SEC_ssurf) && (v.sw.shadow_mask & 2))
		{ // ... a hit of a sphere takes them from that sphere's surface patch (shade_common.h shadow_cands)
			p.shadow_surface_word = (uint32_t) ((s.first[SKR_SEC_ssurf] - s.first[SKR_SEC_smask]) * 4); // (rows of 4 words; the patches follow the masks in the blob)
			p.shadow_surface_stride = s.ssurf_stride;
		}
	}
	if(s.has(SKR_SEC_gi) && v.sw.gi_mask)
	{ // the node pipeline's closest-hit walk of a GI child visits only the spheres its masks name (wave_common.h closest_pair)
		p.gi_index = reinterpret_cast<const int32_t *>(v.sec(SKR_SEC_gi));
		p.gi_masks = reinterpret_cast<const uint32_t *>(v.sec(SKR_SEC_gi)) + s.gi_mask_word;
		p.gi_grid[0] = s.gi_grid[0];
		p.gi_grid[1] = s.gi_grid[1];
		p.gi_wide = s.gi_wide;
		p.gi_all = p.n_spheres >= 32 ? ~0u : (1u << p.n_spheres) - 1u;
		if(s.gi_surface_word && v.sw.gi_surface) p.gi_surface = reinterpret_cast<const uint32_t *>(v.sec(SKR_SEC_gi)) + s.gi_surface_word;
	}
	{ // pick the tightest set of chunk spheres whose |d| bound covers this frame's camera rays (GI children stay below 4,
	  // the smallest bound): primary directions are dir + u right + v up (main.cpp:154-155)
		auto len3 = [](const float *v) { return std::sqrt((double) v[0] * v[0] + (double) v[1] * v[1] + (double) v[2] * v[2]); };
		const double umax = std::fabs((double) p.angle * p.aspect) * 1.001, vmax = std::fabs((double) p.angle) * 1.001;
		const double dmax = len3(c + 3) + umax * len3(c + 9) + vmax * len3(c + 6);
		const double bound[SKR_CULL_LEVELS] = SKR_CULL_DMAX_LIST;
		int level = 0;
		while(level < SKR_CULL_LEVELS && !(dmax < bound[level])) level++;
		p.n_tri_chunks = (level < SKR_CULL_LEVELS && !v.sw.no_cull) ? s.n_chunks : 0;
		if(p.n_tri_chunks) p.tri_chunks += (size_t) level * s.chunk_stride;
	}
	p.monte_carlo = opt->monte_carlo ? 1 : 0;
	p.num_path_traces = opt->num_path_traces;
	p.max_depth = opt->max_depth;
	p.use_shadows = opt->use_shadows ? 1 : 0;
	p.pow_steps = s.pow_steps;
	p.sw.pow_any = (uint16_t) s.pow_any; // (host side: what skr_leaf_pow_plan reads)
	// shade() only recurses under --gillum and only below a sphere hit (raytrace.h:208-218), and with N = 0 there is no
	// child to recurse into: every --depth is then the depth-1 image
	// (--shade-triangles: a triangle hit recurses too)
	p.shade_triangles = (opt->shade_triangles && p.n_tris > 0) ? 1 : 0;
	p.tri_mats = v.sec(SKR_SEC_tri_mats);
	// Only a sphere hit has the terms of raytrace.h:45-103, so a scene without spheres has nothing to add — but the flag also sets the
	// arity of the counter RNG's node ids (N + 2 L, include/skr.h), and a tree over triangle surfaces (--shade-triangles --gillum) has
	// nodes whatever the scene holds: there the flag stays, the legacy children simply never exist (found by tests/fuzz_parity.py:
	// with the flag folded away the node ids from the fourth level down were numbered with arity N)
	p.legacy_reflect = (opt->legacy_reflect && (p.n_spheres > 0 || p.shade_triangles)) ? 1 : 0;
	if(!p.legacy_reflect && (!p.monte_carlo || (p.n_spheres == 0 && !p.shade_triangles) || p.num_path_traces == 0)) p.max_depth = 1;
	if(p.max_depth > 1)
	{ // tree node ids are 32-bit RNG counter words: need N^(depth-1) < 2^32
		double nodes = 1;
		const double arity = skr_tree_arity(p);
		for(int k = 1; k < p.max_depth && nodes < 4294967296.0; k++) nodes = nodes * arity + 1;
		if(nodes >= 4294967296.0)
		{
			skr_set_error("gillum %d at depth %d needs more than 2^32 tree nodes per sample", p.num_path_traces, p.max_depth);
			return SKR_ERR_UNSUPPORTED;
		}
	}
	// --scn-fog: a scene with fog volumes renders on the general level pipeline (render_kernel.hip skr_plan_launch)
	p.n_fog = s.n_fog;
	p.fog_row = (uint32_t) s.first[SKR_SEC_fog];
	// what the scene and the options switch on of the general level pipeline, and whether they go together (launch.h)
	f = generic_features(v, p, query);
	if(const char *why = skr_features_conflict(f, opt->legacy_reflect != 0, opt->shade_triangles != 0, p.n_fog > 0))
	{
		skr_set_error("%s", why);
		return SKR_ERR_UNSUPPORTED;
	}
	p.counters = v.counters;
	p.tri_work = v.count_tri ? v.tri_work : nullptr;
	p.qctr = reinterpret_cast<uint32_t *>(v.counters + CTR_READ_WORDS);
	return SKR_OK;
}

// A launch the device cannot take: not one band of its tables fits the scratch budget (a band holds at least one output row, or the
// `rays` of one row of a shading query), or its kernels need `lds` bytes of LDS, more than a workgroup has
static int check_plan(const skr_renderer *r, const RenderParams &p, bool fits, size_t lds, uint32_t rays)
{
	if(!fits)
	{
		char band[32] = "one output row";
		if(rays) snprintf(band, sizeof band, "%u rays", rays);
		skr_set_error("--depth %d with %d children per node: the tables of %s exceed the scratch budget (SKR_LEVELS_BUDGET_MB)", p.max_depth,
					  p.num_path_traces + (p.legacy_reflect ? 2 * p.n_lights : 0), band);
		return SKR_ERR_UNSUPPORTED;
	}
	if(lds > (size_t) r->scene->lds_limit)
	{
		skr_set_error("scene needs %zu bytes of LDS (%d spheres, %d lights); the device allows %d per workgroup%s", lds, p.n_spheres, p.n_lights,
					  r->scene->lds_limit, r->scene->layout.sphere_tree ? "" : " (the sphere tree, skr_scene_set_sphere_tree / --sphere-tree, keeps the spheres out of LDS)");
		return SKR_ERR_UNSUPPORTED;
	}
	return SKR_OK;
}

// the scene's lens for the kernels that form camera rays alone (launch.h Lens; no trees); null: the pinhole
static const Lens *camera_lens(const SceneLayout &s, Lens &lens)
{
	if(!(s.lens_A > 0.0f)) return nullptr;
	lens = Lens{s.lens_A, s.lens_k, QueryTrees{}};
	return &lens;
}

// the trees a query may walk under the renderer's switches (launch.h QueryTrees)
static QueryTrees query_trees(const LaunchScene &v)
{
	const SceneLayout &s = v.layout;
	QueryTrees q{};
	q.tree = v.sec(SKR_SEC_chunks);
	q.trace = s.has(SKR_SEC_trace) ? v.sec(SKR_SEC_trace) : nullptr;
	q.stride = (uint32_t) s.chunk_stride;
	q.nchunks = v.sw.no_cull ? 0 : s.n_chunks;
	q.cones = (s.cones && !v.sw.no_cones) ? 1 : 0;
	q.trace_cones = (s.trace_cones && !v.sw.no_cones) ? 1 : 0;
	q.ball = ball4(s.trace_ball);
	return q;
}

// the sphere tree of a renderer whose scene had the switch on, under the renderer's switches (render_params.h SphereTree)
static SphereTree sphere_tree_of(const LaunchScene &v)
{
	const SceneLayout &s = v.layout;
	SphereTree t{};
	t.nodes = v.sec(SKR_SEC_st_nodes);
	t.chunks = v.sec(SKR_SEC_st_chunks);
	t.rows = v.sec(SKR_SEC_st_rows);
	t.n_nodes = s.st_nodes;
	t.n_chunks = s.st_chunks;
	t.n_always = s.st_always;
	t.cull = (v.sw.no_sphere_cull || !(s.st_ball.w >= 0.0f)) ? 0 : 1; // (a ball of radius -1: the tree's bounds do not hold, no wave walks it)
	t.ball = ball4(s.st_ball);
	t.work = v.count_tri ? v.st_work : nullptr;
	return t;
}

// The features of a launch on the general level pipeline (launch.h GenericFeatures).  Triangle shadows are in force iff the renderer's
// scene has them switched on, the launch shades triangles (the option is set and the scene has some) and casts shadow rays (include/skr.h
// skr_scene_set_triangle_shadows); otherwise the launch is the one it was without the switch: the same kernels, the same
// skr_kernel_variant().
static GenericFeatures generic_features(const LaunchScene &v, const RenderParams &p, bool query)
{
	const SceneLayout &s = v.layout;
	GenericFeatures f;
	f.tri_shadows = s.tri_shadows && p.shade_triangles && p.use_shadows;
	f.sphere_tree = s.sphere_tree;
	f.spot = s.n_spot > 0;
	f.soft = s.soft;
	if(f.tri_shadows) f.shadows.trees = query_trees(v);
	if(f.sphere_tree) f.stree = sphere_tree_of(v);
	if(f.spot || f.soft) f.spots = SpotLights{v.sec(SKR_SEC_spot), s.spot_first, s.n_spot}; // (n = 0 without spot lights)
	if(f.soft) f.softs = SoftLights{reinterpret_cast<const float *>(v.sec(SKR_SEC_radii)), s.n_radii};
	f.lens = s.lens_A > 0.0f && !query;
	if(f.lens) f.thin_lens = Lens{s.lens_A, s.lens_k, query_trees(v)};
	f.motion = s.motion && p.n_spheres > 0; // (frames and shading queries alike: the shutter time of a query ray is its key's)
	if(f.motion)
	{ // such a launch always carries the spot and radius tables, n = 0 where the scene has none (render_generic.hip with_pack)
		f.mot = Motion{v.vel, s.shutter, query_trees(v)};
		f.spots = SpotLights{v.sec(SKR_SEC_spot), s.spot_first, s.n_spot};
		f.softs = SoftLights{reinterpret_cast<const float *>(v.sec(SKR_SEC_radii)), s.n_radii};
	}
	f.env = s.env_edge > 0; // (frames and shading queries alike)
	if(f.env) f.envmap = EnvMap{v.env, s.env_edge};
	f.tex = s.textured && p.n_spheres > 0; // (frames and shading queries alike)
	f.emit = s.emissive && p.n_spheres > 0; // (frames and shading queries alike)
	if(f.emit) f.emission = Emission{v.emit};
	if(f.tex || f.emit)
	{ // such a launch carries the spot and radius tables too, as one with motion does (render_generic.hip with_pack); one with emission the texture rows
		f.textures = Textures{v.tex + v.tex_rows, reinterpret_cast<const uint2 *>(v.tex)};
		f.spots = SpotLights{v.sec(SKR_SEC_spot), s.spot_first, s.n_spot};
		f.softs = SoftLights{reinterpret_cast<const float *>(v.sec(SKR_SEC_radii)), s.n_radii};
	}
	return f;
}

// one pass of the tiles `ts` selects (render_impl has checked the arguments and set the device)
static int render_pass(skr_renderer *r, const skr_options *opt, uint32_t tile_rows, const TileSel &ts, uint8_t *d_rgb, float *d_rgbf, void *stream)
{
	RenderParams p = camera_params(r->scene->info, opt, opt->seed, 0);
	p.tile_rows = tile_rows;
	p.first_tile = ts.first;
	p.tile_table = ts.d_table;
	p.tile_stride = ts.stride;
	p.out_rows = sel_tiles(opt, tile_rows, ts) * tile_rows;
	p.band_row0 = 0;
	p.band_rows = p.out_rows;
	GenericFeatures f;
	int rc = launch_params(launch_scene(r), opt, p, f);
	if(rc != SKR_OK) return rc;
	p.rgb = d_rgb;
	p.rgbf = d_rgbf;
	LaunchPlan lp;
	const bool fits = skr_plan_launch(p, (size_t) r->scene->lds_limit, lp, f);
	rc = check_plan(r, p, fits, lp.lds_bytes, 0);
	bool kept = false;
	if(rc == SKR_OK && lp.path != SKR_PATH_DIRECT) rc = take_node_scratch(r, lp.scratch_bytes, &kept);
	if(rc == SKR_OK) rc = r->acc.grow(lp.acc_bytes);
	if(rc != SKR_OK) return rc;
	if(lp.path != SKR_PATH_DIRECT) p.node_scratch = r->nodes.p;
	// frames of one camera share the node pipeline's level-0 stage: replay it if the scratch still holds it under this launch's key
	PrimaryKey key;
	const bool keeps = lp.path == SKR_PATH_NODES && skr_primary_key(p, lp.nodes, ts.table_id, key);
	if(keeps) lp.nodes.level0 = kept && !memcmp(&key, &r->level0_key, sizeof key) ? SKR_LEVEL0_REPLAY : SKR_LEVEL0_BUILD;
	if(lp.acc_bytes) p.acc = static_cast<float *>(r->acc.p);
	SkrTimingHook hook;
	if(r->timing)
	{
		if(!r->free_pairs.empty())
		{
			hook = r->free_pairs.back();
			r->free_pairs.pop_back();
		}
		else
		{
			SKR_HIP(hipEventCreate(&hook.start));
			SKR_HIP(hipEventCreate(&hook.stop));
		}
		if(!r->d_snap)
		{
			SKR_HIP(hipMalloc((void **) &r->d_snap, CTR_SNAP_BYTES));
			SKR_HIP(hipMemset(r->d_snap, 0, CTR_SNAP_BYTES));
		}
		hook.snap = r->d_snap;
		hook.counters = r->scene->d_counters;
	}
	r->last_off_ctr = lp.off_ctr;
	r->last_levels = lp.levels;
	r->last_leaf_shape = (lp.path == SKR_PATH_NODES && !lp.nodes.flat) ? (int) skr_leaf_shape(p) : -1; // (what launch_leaf2, render_nodes.hip, asks too)
	r->last_leaf_pow = r->last_leaf_shape >= 0 ? (int) skr_leaf_pow_plan(p) : -1;
	g_variant = lp.variant;
	SKR_HIP(skr_launch_render(p, lp, (hipStream_t) stream, r->timing ? &hook : nullptr));
	if(r->timing) r->timed.push_back(hook);
	if(keeps)
	{ // (only behind a launch that went through)
		r->level0_key = key;
		r->level0_kept = true;
		(lp.nodes.level0 == SKR_LEVEL0_REPLAY ? r->level0_replays : r->level0_builds)++;
	}
	return SKR_OK;
}

// the progressive passes' scratch for frames of n floats: this pass's frame | the running sum
static int progressive_scratch(skr_renderer *r, size_t n, float *&frame, float *&acc)
{
	const int rc = r->prog.grow(2 * n * sizeof(float));
	frame = static_cast<float *>(r->prog.p);
	acc = frame + n;
	return rc;
}

// the options of pass k of a multi-pass render: one frame under the seed s + k
static skr_options pass_options(const skr_options *opt, uint64_t k)
{
	skr_options pass = *opt;
	pass.progressive_passes = 1;
	pass.seed = opt->seed + k;
	return pass;
}

// skr_options.progressive_passes: K frames under the seeds s, s+1, ..., s+K-1, summed in binary32 in pass
// order, divided by K once and quantised like a single frame (accumulate.hip).  K <= 1 is the single frame itself.
static int render_impl(skr_renderer *r, const skr_options *opt, uint32_t tile_rows, const TileSel &ts, uint8_t *d_rgb, float *d_rgbf, void *stream)
{
	if(!r || !opt || (!d_rgb && !d_rgbf) || tile_rows == 0 || ts.stride == 0)
	{
		skr_set_error("skr_render_tiles: bad argument");
		return SKR_ERR_ARG;
	}
	int rc = check_options(opt);
	if(rc != SKR_OK) return rc;
	const uint32_t n_tiles = sel_tiles(opt, tile_rows, ts);
	if(n_tiles == 0) return SKR_OK;
	SKR_HIP(hipSetDevice(r->scene->device));
	if(opt->progressive_passes <= 1) return render_pass(r, opt, tile_rows, ts, d_rgb, d_rgbf, stream);
	const uint32_t out_rows = n_tiles * tile_rows;
	const size_t n = (size_t) opt->width * out_rows * 3;
	float *frame, *acc;
	rc = progressive_scratch(r, n, frame, acc);
	if(rc != SKR_OK) return rc;
	for(int32_t k = 0; k < opt->progressive_passes; k++)
	{
		const skr_options pass = pass_options(opt, (uint64_t) k);
		rc = render_pass(r, &pass, tile_rows, ts, nullptr, frame, stream);
		if(rc != SKR_OK) return rc;
		SKR_HIP(skr_launch_accumulate(acc, frame, n, k == 0, (hipStream_t) stream));
	}
	SKR_HIP(skr_launch_resolve_accumulated(acc, (uint32_t) opt->progressive_passes, (uint32_t) opt->width, out_rows, (uint32_t) opt->height, tile_rows, ts.first,
										   ts.stride, ts.d_table, d_rgb, d_rgbf, (hipStream_t) stream));
	return SKR_OK;
}

int skr_render_tiles(skr_renderer *r, const skr_options *opt, uint32_t tile_rows, uint32_t first_tile, uint32_t tile_stride,
					 uint8_t *d_rgb, float *d_rgbf, void *stream)
{
	TileSel ts;
	ts.first = first_tile;
	ts.stride = tile_stride;
	return render_impl(r, opt, tile_rows, ts, d_rgb, d_rgbf, stream);
}

int skr_render_tile_list(skr_renderer *r, const skr_options *opt, uint32_t tile_rows, const uint32_t *d_tiles, uint32_t n_slots, uint8_t *d_rgb, float *d_rgbf, void *stream)
{
	return skr_render_tile_list_owned(r, opt, tile_rows, d_tiles, n_slots, 0, d_rgb, d_rgbf, stream); // (0: contents unknown — such a launch never replays a level-0 stage)
}

int skr_renderer_primary_cache_stats(skr_renderer *r, uint64_t *builds, uint64_t *replays)
{
	if(!r) return SKR_ERR_ARG;
	if(builds) *builds = r->level0_builds;
	if(replays) *replays = r->level0_replays;
	return SKR_OK;
}

// Internal (not in include/skr.h: tests only).  The shape whose instance of the leaf kernel the launch last enqueued ran (launch.h
// SkrLeafShape: 0 = the instance that reads every fact at run time); -1: that launch ran no leaf kernel (another path, the flat schedule).
int skr_renderer_last_leaf_shape(const skr_renderer *r) { return r ? r->last_leaf_shape : -1; }
// ... and the exponent mask of that instance (launch.h skr_leaf_pow_plan: 0 = the run-time instance, which has none); -1 as above
int skr_renderer_last_leaf_pow(const skr_renderer *r) { return r ? r->last_leaf_pow : -1; }

// Internal (tests only; no device involved): skr_leaf_shape (launch.h) of the launch that a renderer of `scene` would make for `opt`
// under the SKR_* switches of the environment as it is now — launch_params on the packed scene, nothing uploaded.  < 0: minus an error code.
// what: 0 = skr_leaf_shape, 1 = skr_leaf_pow_plan
static int scene_leaf_plan(const skr_scene *scene, const skr_options *opt, int what)
{
	if(!scene || !opt) return -SKR_ERR_ARG;
	SceneLayout layout;
	const std::vector<skr_f4> rows = skr_pack_scene(*scene, layout);
	std::vector<unsigned long long> counters(CTR_READ_WORDS + CTR_RESERVED_WORDS);
	SkrSwitches sw;
	load_switches(sw);
	RenderParams p = camera_params(scene->info, opt, opt->seed, 0);
	GenericFeatures f; // (host memory: only addresses are formed, and null-ness asked)
	const LaunchScene v{scene->info, layout, reinterpret_cast<const float4 *>(rows.data()), nullptr, counters.data(), nullptr, nullptr, sw, false, reinterpret_cast<const float4 *>(rows.data()), reinterpret_cast<const float4 *>(rows.data()), reinterpret_cast<const float4 *>(rows.data()), 0, reinterpret_cast<const float4 *>(rows.data())};
	const int rc = launch_params(v, opt, p, f);
	return rc != SKR_OK ? -rc : what ? (int) skr_leaf_pow_plan(p) : (int) skr_leaf_shape(p);
}
int skr_scene_leaf_shape(const skr_scene *scene, const skr_options *opt) { return scene_leaf_plan(scene, opt, 0); }
// Internal (tests only; no device involved), as skr_scene_leaf_shape: the exponent mask of the leaf kernel's instance for that launch
// (launch.h skr_leaf_pow_plan): 0 where the launch gets the run-time instance.  < 0: minus an error code.
int skr_scene_leaf_pow(const skr_scene *scene, const skr_options *opt) { return scene_leaf_plan(scene, opt, 1); }

// Per tile of `tile_rows` image rows: the work its pixels cost, counted — the tile is rendered on its own and the work counters read
// (radiance rays, shaded hits, ray-sphere tests as the reference's loops run them), priced in flops like bench.py prices a frame
// (34 per ray-sphere test, 150 per shaded hit; a ray through a triangle mesh walks ~6 chunk spheres and ~5 triangles).
// Integer counts of a bit-reproducible render: every rank of a job computes the same numbers.  Synchronous, one small render per tile
// (tens of milliseconds for a 1080p frame: the frame steps do it once per frame geometry); the caller's work counters are preserved.
int skr_tile_costs(skr_renderer *r, const skr_options *opt, uint32_t tile_rows, uint64_t *h_cost)
{
	if(!r || !opt || !h_cost || tile_rows == 0) return SKR_ERR_ARG;
	int rc = check_options(opt);
	if(rc != SKR_OK) return rc;
	SKR_HIP(hipSetDevice(r->scene->device));
	const uint32_t T = ((uint32_t) opt->height + tile_rows - 1) / tile_rows;
	SKR_HIP(hipDeviceSynchronize()); // (frames still in flight on other streams add to the counters this probe borrows)
	std::vector<unsigned long long> saved(CTR_READ_WORDS);
	SKR_HIP(hipMemcpy(saved.data(), r->scene->d_counters, saved.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
	SKR_HIP(hipMemset(r->scene->d_counters, 0, saved.size() * sizeof(unsigned long long)));
	std::vector<uint32_t> tiles(T);
	for(uint32_t t = 0; t < T; t++) tiles[t] = t;
	uint32_t *d_tiles = nullptr;
	uint8_t *d_rgb = nullptr;
	hipError_t e = hipMalloc((void **) &d_tiles, (size_t) T * sizeof(uint32_t));
	if(e == hipSuccess) e = hipMalloc((void **) &d_rgb, (size_t) tile_rows * (size_t) opt->width * 3);
	if(e == hipSuccess) e = hipMemcpy(d_tiles, tiles.data(), (size_t) T * sizeof(uint32_t), hipMemcpyHostToDevice);
	const bool was_counting = r->count_tri, was_timing = r->timing; // the probe's launches are not the caller's: they count no walk work and are not timed
	r->count_tri = false;
	r->timing = false;
	for(uint32_t t = 0; t < T && e == hipSuccess && rc == SKR_OK; t++)
	{
		rc = skr_render_tile_list(r, opt, tile_rows, d_tiles + t, 1, d_rgb, nullptr, nullptr);
		uint64_t w[4] = {0, 0, 0, 0};
		if(rc == SKR_OK) rc = skr_renderer_read_work(r, w, 1);
		const uint64_t mesh = r->scene->info.n_triangles > 64 ? (uint64_t) (6 * 19 + 5 * 46) : (uint64_t) r->scene->info.n_triangles * 46;
		h_cost[t] = 34 * w[3] + 150 * w[1] + (20 + mesh) * (w[0] + w[2]);
	}
	r->count_tri = was_counting;
	r->timing = was_timing;
	if(d_tiles) (void) hipFree(d_tiles);
	if(d_rgb) (void) hipFree(d_rgb);
	if(e == hipSuccess) e = hipMemcpy(r->scene->d_counters, saved.data(), saved.size() * sizeof(unsigned long long), hipMemcpyHostToDevice);
	if(e != hipSuccess)
	{
		skr_set_error("skr_tile_costs: %s", hipGetErrorString(e));
		return SKR_ERR_HIP;
	}
	return rc;
}

int skr_accumulate(float *d_acc, const float *d_frame, uint64_t n_floats, int first, void *stream)
{
	if(!d_acc || !d_frame)
	{
		skr_set_error("skr_accumulate: null argument");
		return SKR_ERR_ARG;
	}
	SKR_HIP(skr_launch_accumulate(d_acc, d_frame, (size_t) n_floats, first, (hipStream_t) stream));
	return SKR_OK;
}

int skr_resolve_accumulated(const float *d_acc, uint32_t passes, uint32_t width, uint32_t height, uint8_t *d_rgb, float *d_rgbf, void *stream)
{
	if(!d_acc || passes == 0 || (!d_rgb && !d_rgbf))
	{
		skr_set_error("skr_resolve_accumulated: bad argument");
		return SKR_ERR_ARG;
	}
	SKR_HIP(skr_launch_resolve_accumulated(d_acc, passes, width, height, height, height ? height : 1, 0, 1, nullptr, d_rgb, d_rgbf, (hipStream_t) stream));
	return SKR_OK;
}

int skr_render_rows(skr_renderer *r, const skr_options *opt, uint32_t y0, uint32_t y1, uint8_t *d_rgb, float *d_rgbf, void *stream)
{
	if(!opt || y1 <= y0 || y1 > (uint32_t) opt->height)
	{
		skr_set_error("skr_render_rows: bad row range [%u,%u)", y0, y1);
		return SKR_ERR_ARG;
	}
	// rows [y0,y1) = consecutive tiles of g = gcd(y0, y1-y0) rows starting at tile y0/g
	uint32_t a = y0, b = y1 - y0;
	while(b)
	{
		const uint32_t t = a % b;
		a = b;
		b = t;
	}
	TileSel ts;
	ts.first = y0 / a;
	ts.stride = 1;
	ts.max_tiles = (y1 - y0) / a;
	return render_impl(r, opt, a, ts, d_rgb, d_rgbf, stream);
}

int skr_renderer_reload_switches(skr_renderer *r)
{
	if(!r) return SKR_ERR_ARG;
	load_switches(r->sw);
	return SKR_OK;
}

int skr_renderer_kernel_timing(skr_renderer *r, int enable)
{
	if(!r) return SKR_ERR_ARG;
	r->timing = enable != 0;
	return SKR_OK;
}

int skr_renderer_kernel_ms(skr_renderer *r, float *mean_ms, int32_t *launches)
{
	if(!r || !mean_ms) return SKR_ERR_ARG;
	SKR_HIP(hipSetDevice(r->scene->device));
	double sum = 0;
	int n = 0;
	for(SkrTimingHook &h : r->timed)
	{
		SKR_HIP(hipEventSynchronize(h.stop));
		float ms = 0;
		SKR_HIP(hipEventElapsedTime(&ms, h.start, h.stop));
		sum += ms;
		n++;
		r->free_pairs.push_back(h);
	}
	r->timed.clear();
	*mean_ms = n ? (float) (sum / n) : 0.0f;
	if(launches) *launches = n;
	return SKR_OK;
}

// node pipeline: records of level `level` in the band last rendered (level 0: its level-0 nodes)
static int nodes_level_count(skr_renderer *r, int level, uint32_t *n)
{
	if(!r || !n) return SKR_ERR_ARG;
	SKR_HIP(hipSetDevice(r->scene->device));
	*n = 0;
	if(level < r->last_levels) SKR_HIP(skr_nodes_level_count(r->nodes.p, r->last_off_ctr, level, n)); // (only the node pipeline has level tables of this layout)
	return SKR_OK;
}

int skr_renderer_last_parent_count(skr_renderer *r, uint32_t *n) { return nodes_level_count(r, 0, n); }

int skr_renderer_last_level1_count(skr_renderer *r, uint32_t *n) { return nodes_level_count(r, 1, n); }

static int read_work(skr_renderer *r, uint64_t *out, int n_out, int reset)
{
	if(!r || !out) return SKR_ERR_ARG;
	SKR_HIP(hipSetDevice(r->scene->device));
	// the work counters and (diagnostic builds) the phase stamps behind them; the queue counters that follow are not touched
	std::vector<unsigned long long> h(CTR_READ_WORDS);
	SKR_HIP(hipMemcpy(h.data(), r->scene->d_counters, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost)); // synchronises with prior launches
	for(int k = 0; k < n_out; k++) out[k] = 0;
	for(size_t s = 0; s < CTR_WORK_WORDS; s += 4)
		for(int k = 0; k < n_out; k++) out[k] += h[s + k];
	if(getenv("SKR_PRINT_STAMPS"))
	{ // diagnostic builds (-DSKR_STAMPS=1) only: per-phase cycle sums
		for(size_t k = 0; k < CTR_STAMP_WORDS; k++) fprintf(stderr, "stamp[%zu] = %llu\n", k, h[CTR_WORK_WORDS + k]);
	}
	// (null stream: callers read the counters between frames, after synchronising their render stream)
	if(reset) SKR_HIP(hipMemset(r->scene->d_counters, 0, h.size() * sizeof(unsigned long long)));
	return SKR_OK;
}

int skr_renderer_read_counters(skr_renderer *r, uint64_t out[3], int reset) { return read_work(r, out, 3, reset); }

int skr_renderer_read_work(skr_renderer *r, uint64_t out[4], int reset)
{
	const int rc = read_work(r, out, 4, reset);
	if(rc != SKR_OK) return rc;
	// every radiance ray tests every sphere (raytrace.h:152-165); a shadow ray stops at its first occluder (utils.h:52-55)
	out[3] += out[0] * (uint64_t) r->scene->info.n_spheres;
	return SKR_OK;
}

int skr_renderer_count_triangle_work(skr_renderer *r, int enable)
{
	if(!r) return SKR_ERR_ARG;
	r->count_tri = enable != 0;
	return SKR_OK;
}

int skr_renderer_kernel_work(skr_renderer *r, uint64_t out[4])
{
	if(!r || !out) return SKR_ERR_ARG;
	for(int k = 0; k < 4; k++) out[k] = 0;
	if(!r->d_snap) return SKR_OK;
	SKR_HIP(hipSetDevice(r->scene->device));
	std::vector<unsigned long long> h(2 * CTR_WORK_WORDS);
	SKR_HIP(hipMemcpy(h.data(), r->d_snap, CTR_SNAP_BYTES, hipMemcpyDeviceToHost)); // synchronises with prior launches
	for(size_t s = 0; s < CTR_WORK_WORDS; s += 4)
		for(int k = 0; k < 4; k++) out[k] += h[CTR_WORK_WORDS + s + k] - h[s + k];
	out[3] += out[0] * (uint64_t) r->scene->info.n_spheres; // (as skr_renderer_read_work)
	return SKR_OK;
}

// the counters of a walk (d_tri_work, d_st_work), summed over their shards: {culling-sphere tests, leaf tests}
static int read_walk_work(unsigned long long *d_work, uint64_t out[2], int reset)
{
	unsigned long long h[WALK_SHARDS * 2];
	SKR_HIP(hipMemcpy(h, d_work, WALK_BYTES, hipMemcpyDeviceToHost)); // synchronises with prior launches
	for(size_t s = 0; s < WALK_SHARDS; s++)
	{
		out[0] += h[2 * s];
		out[1] += h[2 * s + 1];
	}
	if(reset) SKR_HIP(hipMemset(d_work, 0, WALK_BYTES));
	return SKR_OK;
}

int skr_renderer_read_triangle_work(skr_renderer *r, uint64_t out[3], int reset)
{
	if(!r || !out) return SKR_ERR_ARG;
	uint64_t w[4];
	const int rc = read_work(r, w, 4, 0);
	if(rc != SKR_OK) return rc;
	out[0] = out[1] = 0;
	out[2] = w[0] * (uint64_t) r->scene->info.n_triangles; // raytrace.h:171-186: every radiance ray tests every triangle
	return read_walk_work(r->scene->d_tri_work, out, reset);
}

int skr_renderer_read_sphere_tree_work(skr_renderer *r, uint64_t out[2], int reset)
{
	if(!r || !out) return SKR_ERR_ARG;
	out[0] = out[1] = 0;
	if(!r->scene->d_st_work) return SKR_OK; // (no sphere tree: no walks)
	SKR_HIP(hipSetDevice(r->scene->device));
	return read_walk_work(r->scene->d_st_work, out, reset);
}

int skr_render_progressive_host(skr_renderer *r, const skr_options *opt, uint32_t every, uint8_t *h_rgb, float *h_rgbf, skr_progress_fn progress, void *user,
								float *kernel_ms)
{
	if(!r || !opt || (!h_rgb && !h_rgbf))
	{
		skr_set_error("skr_render_progressive_host: bad argument");
		return SKR_ERR_ARG;
	}
	int rc = check_options(opt); // before anything is sized from width x height
	if(rc != SKR_OK) return rc;
	SKR_HIP(hipSetDevice(r->scene->device));
	const size_t n = (size_t) opt->width * opt->height * 3; // (the frame's bytes, its floats)
	HostFrame f;
	rc = host_frame(r, n / 3, false, f);
	if(rc != SKR_OK) return rc;
	float *d_rgbf = h_rgbf ? f.rgbf : nullptr;
	const uint32_t passes = opt->progressive_passes > 1 ? (uint32_t) opt->progressive_passes : 1u;
	if(!progress || every == 0 || every >= passes)
	{ // nobody looks before the end: the frame (or the K-pass mean) in one launch sequence
		rc = timed_host(r, [&] { return skr_render_tiles(r, opt, (uint32_t) opt->height, 0, 1, f.rgb, d_rgbf, nullptr); },
						{{h_rgb, f.rgb, n}, {h_rgbf, d_rgbf, n * 4}}, kernel_ms);
		if(rc == SKR_OK && progress) (void) progress(user, passes, passes, h_rgb, h_rgbf);
		return rc;
	}
	// the mean is shown while it forms: after every `every` passes (and after the last) it is resolved, copied out and handed to
	// the callback — where the SDL viewer of main.cpp:183-197 would blit.  The final mean is the one-launch result, bit for bit.
	float *frame, *acc;
	rc = progressive_scratch(r, n, frame, acc);
	if(rc != SKR_OK) return rc;
	float total_ms = 0;
	for(uint32_t k = 0; k < passes; k++)
	{
		const skr_options pass = pass_options(opt, k);
		const bool show = (k + 1) % every == 0 || k + 1 == passes;
		const uint32_t h = (uint32_t) opt->height;
		float ms = 0;
		rc = timed_host(r, [&]() -> int {
			const int e = render_pass(r, &pass, h, TileSel(), nullptr, frame, nullptr);
			if(e != SKR_OK) return e;
			SKR_HIP(skr_launch_accumulate(acc, frame, n, k == 0, nullptr));
			if(show) SKR_HIP(skr_launch_resolve_accumulated(acc, k + 1, (uint32_t) opt->width, h, h, h, 0, 1, nullptr, f.rgb, d_rgbf, nullptr));
			return SKR_OK;
		}, {{show ? h_rgb : nullptr, f.rgb, n}, {show ? h_rgbf : nullptr, d_rgbf, n * 4}}, &ms);
		if(rc != SKR_OK) return rc;
		total_ms += ms;
		if(show && progress(user, k + 1, passes, h_rgb, h_rgbf) != 0) break; // the viewer was closed: what is in the buffers is the mean so far
	}
	if(kernel_ms) *kernel_ms = total_ms;
	return SKR_OK;
}

int skr_render_frame_host(skr_renderer *r, const skr_options *opt, uint8_t *h_rgb, float *kernel_ms)
{
	if(!h_rgb) return SKR_ERR_ARG;
	return skr_render_progressive_host(r, opt, 0, h_rgb, nullptr, nullptr, nullptr, kernel_ms);
}

const char *skr_kernel_variant(void) { return g_variant; }

// ---- ray queries (trace_rays.hip): they read the scene blob and write only the caller's arrays ----
int skr_trace_rays(skr_renderer *r, const skr_ray *d_rays, uint32_t n, uint32_t flags, void *d_out, void *stream)
{
	const bool any_hit = (flags & SKR_TRACE_ANY_HIT) != 0;
	if(!r || !d_rays || !d_out || (flags & ~SKR_TRACE_ANY_HIT) || ((uintptr_t) d_rays & 15) || ((uintptr_t) d_out & (any_hit ? 3 : 15)))
	{
		skr_set_error("skr_trace_rays: bad argument (null or misaligned array, or unknown flags 0x%x)", flags);
		return SKR_ERR_ARG;
	}
	if(n == 0) return SKR_OK;
	const DeviceScene &sc = *r->scene;
	SKR_HIP(hipSetDevice(sc.device));
	TraceScene s{};
	const LaunchScene v = launch_scene(r);
	s.geom = v.blob;
	s.tris = v.sec(SKR_SEC_tris);
	s.ns = sc.info.n_spheres;
	s.nt = sc.info.n_triangles;
	s.chunk = sc.layout.chunk_size;
	s.cam = f3{sc.info.camera[0], sc.info.camera[1], sc.info.camera[2]};
	s.trees = query_trees(v);
	SphereTree st{};
	if(sc.layout.sphere_tree)
	{ // the sphere searches walk the tree (a query counts nothing)
		st = sphere_tree_of(v);
		st.work = nullptr;
	}
	SKR_HIP(skr_launch_trace(s, reinterpret_cast<const float4 *>(d_rays), n, any_hit, d_out, (hipStream_t) stream, sc.layout.sphere_tree ? &st : nullptr));
	return SKR_OK;
}

int skr_camera_rays(skr_renderer *r, const skr_options *opt, uint32_t sample, skr_ray *d_rays, void *stream)
{
	if(!r || !opt || !d_rays || ((uintptr_t) d_rays & 15))
	{
		skr_set_error("skr_camera_rays: bad argument (null or misaligned array)");
		return SKR_ERR_ARG;
	}
	int rc = check_options(opt);
	if(rc != SKR_OK) return rc;
	if(sample >= (uint32_t) (opt->grid_size > 0 ? opt->grid_size * opt->grid_size : 1))
	{
		skr_set_error("skr_camera_rays: sample %u of a frame with %d AA samples", sample, opt->grid_size > 0 ? opt->grid_size * opt->grid_size : 1);
		return SKR_ERR_ARG;
	}
	SKR_HIP(hipSetDevice(r->scene->device));
	Lens lens;
	SKR_HIP(skr_launch_camera_rays(camera_params(r->scene->info, opt, opt->seed, sample), reinterpret_cast<float4 *>(d_rays), (hipStream_t) stream, camera_lens(r->scene->layout, lens)));
	return SKR_OK;
}

// ---- shading queries (render_generic.hip): the radiance of caller-supplied rays on the general level pipeline ----
int skr_shade_rays(skr_renderer *r, const skr_options *opt, const skr_ray *d_rays, uint32_t n, uint32_t sample, const uint32_t *d_keys, float *d_rgbf,
				   void *stream)
{
	if(!r || !opt || !d_rays || !d_rgbf || ((uintptr_t) d_rays & 15) || ((uintptr_t) d_rgbf & 3) || ((uintptr_t) d_keys & 3))
	{
		skr_set_error("skr_shade_rays: bad argument (null or misaligned array)");
		return SKR_ERR_ARG;
	}
	int rc = check_options(opt);
	if(rc != SKR_OK) return rc;
	if(n == 0) return SKR_OK;
	SKR_HIP(hipSetDevice(r->scene->device));
	RenderParams p = camera_params(r->scene->info, opt, opt->seed, sample);
	p.width = (int32_t) SKR_SHADE_ROW; // the plan's rows: SKR_SHADE_ROW rays each, the last one partial
	p.tile_rows = 1;
	p.tile_stride = 1;
	p.out_rows = (uint32_t) (((uint64_t) n + SKR_SHADE_ROW - 1) / SKR_SHADE_ROW);
	p.band_rows = p.out_rows;
	GenericFeatures f;
	const LaunchScene v = launch_scene(r);
	rc = launch_params(v, opt, p, f, true);
	if(rc != SKR_OK) return rc;
	p.grid_size = 0; // (one sample: `sample`)
	GPlan pl;
	const bool fits = skr_generic_plan(p, pl, f.sphere_tree);
	rc = check_plan(r, p, fits, f.sphere_tree ? skr_lights_kernels_lds(p) : skr_scene_kernels_lds(p), SKR_SHADE_ROW);
	if(rc == SKR_OK) rc = take_node_scratch(r, pl.total);
	if(rc != SKR_OK) return rc;
	p.node_scratch = r->nodes.p;
	ShadeRays q{};
	q.rays = reinterpret_cast<const float4 *>(d_rays);
	q.keys = d_keys;
	q.out = d_rgbf;
	q.n = n;
	q.trees = query_trees(v);
	r->last_levels = 0; // (the scratch no longer holds the node pipeline's tables of the last render)
	g_variant = skr_generic_variant(true, f);
	SKR_HIP(skr_launch_generic(p, pl, (hipStream_t) stream, nullptr, f, &q));
	return SKR_OK;
}

// ---- the denoiser (denoise.hip): reads the caller's frame and guides, writes only the caller's outputs ----
static bool overlaps(const void *a, size_t na, const void *b, size_t nb)
{
	if(!a || !b) return false;
	const uintptr_t x = (uintptr_t) a, y = (uintptr_t) b;
	return x < y + nb && y < x + na;
}

// skr_denoise and skr_denoise_var: d_var null, or the per-pixel variance image that replaces the spatial estimate where it is measured
static int denoise(skr_renderer *r, const char *who, uint32_t width, uint32_t height, const float *d_rgbf, const skr_hit *d_hits, const float *d_var,
				   uint32_t iterations, float *d_out_rgbf, uint8_t *d_out_rgb, void *stream)
{
	if(!r || !d_rgbf || !d_hits || (!d_out_rgbf && !d_out_rgb) || ((uintptr_t) d_rgbf & 3) || ((uintptr_t) d_hits & 15) || ((uintptr_t) d_out_rgbf & 3) ||
	   ((uintptr_t) d_var & 3))
	{
		skr_set_error("%s: bad argument (null or misaligned array, or no output)", who);
		return SKR_ERR_ARG;
	}
	if(width == 0 || height == 0 || width > 65536 || height > 65536 || iterations > SKR_DENOISE_MAX_ITERATIONS)
	{
		skr_set_error("%s: bad size %ux%u or iterations %u (0 .. %d)", who, width, height, iterations, SKR_DENOISE_MAX_ITERATIONS);
		return SKR_ERR_ARG;
	}
	const size_t n = (size_t) width * height;
	if(overlaps(d_out_rgbf, n * 12, d_rgbf, n * 12) || overlaps(d_out_rgbf, n * 12, d_hits, n * sizeof(skr_hit)) || overlaps(d_out_rgb, n * 3, d_rgbf, n * 12) ||
	   overlaps(d_out_rgb, n * 3, d_hits, n * sizeof(skr_hit)) || overlaps(d_out_rgbf, n * 12, d_out_rgb, n * 3) || overlaps(d_out_rgbf, n * 12, d_var, n * 4) ||
	   overlaps(d_out_rgb, n * 3, d_var, n * 4))
	{
		skr_set_error("%s: an output overlaps an input or the other output", who);
		return SKR_ERR_ARG;
	}
	SKR_HIP(hipSetDevice(r->scene->device));
	ScratchLayout L;
	const size_t o_img0 = L.take(n * sizeof(float4)), o_img1 = L.take(n * sizeof(float4)), o_guide = L.take(n * sizeof(float4)), o_cls = L.take(n * sizeof(uint32_t));
	const int rc = r->dn.grow(L.off);
	if(rc != SKR_OK) return rc;
	const DenoiseScratch b{{r->dn.at<float4>(o_img0), r->dn.at<float4>(o_img1)}, r->dn.at<float4>(o_guide), r->dn.at<uint32_t>(o_cls)};
	SKR_HIP(skr_launch_denoise(b, width, height, d_rgbf, reinterpret_cast<const float4 *>(d_hits), d_var, (int) iterations, d_out_rgbf, d_out_rgb,
							   (hipStream_t) stream));
	return SKR_OK;
}

int skr_denoise(skr_renderer *r, uint32_t width, uint32_t height, const float *d_rgbf, const skr_hit *d_hits, uint32_t iterations, float *d_out_rgbf,
				uint8_t *d_out_rgb, void *stream)
{
	return denoise(r, "skr_denoise", width, height, d_rgbf, d_hits, nullptr, iterations, d_out_rgbf, d_out_rgb, stream);
}

int skr_denoise_var(skr_renderer *r, uint32_t width, uint32_t height, const float *d_rgbf, const skr_hit *d_hits, const float *d_var, uint32_t iterations,
					float *d_out_rgbf, uint8_t *d_out_rgb, void *stream)
{
	return denoise(r, "skr_denoise_var", width, height, d_rgbf, d_hits, d_var, iterations, d_out_rgbf, d_out_rgb, stream);
}

// ---- adaptive sampling (adaptive.hip): extra passes only for the pixels whose estimate is still noisy ----
void skr_adaptive_default(skr_adaptive *a)
{
	if(!a) return;
	a->min_passes = SKR_ADAPTIVE_MIN_PASSES;
	a->max_passes = SKR_ADAPTIVE_MAX_PASSES;
	a->threshold = SKR_ADAPTIVE_THRESHOLD;
	a->reserved = 0;
}

static int check_adaptive(const skr_options *opt, const skr_adaptive *a, const char *who)
{
	if(opt->progressive_passes > 1)
	{
		skr_set_error("%s: progressive_passes %d: adaptive sampling chooses the passes itself (leave it at 1)", who, opt->progressive_passes);
		return SKR_ERR_ARG;
	}
	if(a->min_passes < 1 || a->max_passes < a->min_passes || a->max_passes > SKR_ADAPTIVE_PASS_LIMIT || std::isnan(a->threshold) || a->reserved != 0)
	{
		skr_set_error("%s: need 1 <= min_passes <= max_passes <= %d and a threshold that is not NaN (got %d, %d, %g)", who, SKR_ADAPTIVE_PASS_LIMIT,
					  a->min_passes, a->max_passes, (double) a->threshold);
		return SKR_ERR_ARG;
	}
	int rc = check_options(opt);
	if(rc != SKR_OK) return rc;
	if((uint64_t) opt->width * (uint64_t) opt->height > 0xFFFFFFFFull)
	{
		skr_set_error("%s: %dx%d pixels do not fit the 32-bit pixel lists", who, opt->width, opt->height);
		return SKR_ERR_ARG;
	}
	return SKR_OK;
}

static int render_adaptive(skr_renderer *r, const char *who, const skr_options *opt, const skr_adaptive *a, uint8_t *d_rgb, float *d_rgbf, uint32_t *d_passes,
						   float *d_var, void *stream)
{
	if(!r || !opt || !a || (!d_rgb && !d_rgbf && !d_passes && !d_var) || ((uintptr_t) d_rgbf & 3) || ((uintptr_t) d_passes & 3) || ((uintptr_t) d_var & 3))
	{
		skr_set_error("%s: bad argument (null or misaligned array, or no output)", who);
		return SKR_ERR_ARG;
	}
	int rc = check_adaptive(opt, a, who);
	if(rc != SKR_OK) return rc;
	SKR_HIP(hipSetDevice(r->scene->device));
	const hipStream_t st = (hipStream_t) stream;
	const uint64_t pixels = (uint64_t) opt->width * (uint64_t) opt->height;
	float *frame, *acc; // (the passes are folded into the statistics: the running sum is not used)
	rc = progressive_scratch(r, (size_t) pixels * 3, frame, acc);
	if(rc == SKR_OK) rc = r->ad.grow(skr_adaptive_scratch_bytes(pixels));
	if(rc != SKR_OK) return rc;
	if(!r->h_count) SKR_HIP(hipHostMalloc((void **) &r->h_count, sizeof(uint32_t), hipHostMallocDefault));
	const AdaptiveScratch s = skr_adaptive_carve(r->ad.p, pixels);
	// the first min_passes passes: whole frames
	for(int32_t k = 0; k < a->min_passes; k++)
	{
		const skr_options pass = pass_options(opt, (uint64_t) k);
		rc = render_pass(r, &pass, (uint32_t) opt->height, TileSel(), nullptr, frame, stream);
		if(rc != SKR_OK) return rc;
		SKR_HIP(skr_launch_adaptive_fold(s, frame, nullptr, (uint32_t) pixels, k == 0, st));
	}
	// then one round per pass index n while pixels are active: select (the first list is every pixel), read the count back, one pass
	const AdaptiveRule rule{(uint32_t) a->min_passes, (uint32_t) a->max_passes, a->threshold};
	const uint32_t samples = opt->grid_size > 0 ? (uint32_t) (opt->grid_size * opt->grid_size) : 0u;
	const uint32_t *in = nullptr;
	uint32_t m = (uint32_t) pixels;
	for(uint32_t n = (uint32_t) a->min_passes, cur = 0; n < (uint32_t) a->max_passes; n++, cur ^= 1)
	{
		uint32_t *out = s.list[cur];
		SKR_HIP(skr_launch_adaptive_select(s, rule, in, m, out, st));
		SKR_HIP(hipMemcpyAsync(r->h_count, s.count, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
		SKR_HIP(hipStreamSynchronize(st));
		m = *r->h_count;
		in = out;
		if(m == 0) break;
		const skr_options pass = pass_options(opt, n);
		const bool whole = r->sw.adaptive_path == 1 || (r->sw.adaptive_path == 0 && (double) m >= (double) SKR_ADAPTIVE_CROSSOVER * (double) pixels);
		if(whole)
		{ // frame path: the whole frame, its listed pixels gathered
			rc = render_pass(r, &pass, (uint32_t) opt->height, TileSel(), nullptr, frame, stream);
			if(rc != SKR_OK) return rc;
			SKR_HIP(skr_launch_adaptive_fold(s, frame, in, m, 0, st));
			continue;
		}
		// query path: per AA sample the listed pixels' camera rays, shaded with the pixel words as keys (skr_shade_rays)
		RenderParams p = camera_params(r->scene->info, opt, pass.seed, 0);
		Lens lens;
		const Lens *lp = camera_lens(r->scene->layout, lens);
		for(uint32_t aa = 0; aa < (samples ? samples : 1u); aa++)
		{
			p.aa_index = aa;
			SKR_HIP(skr_launch_adaptive_rays(p, in, m, s.rays, st, lp));
			rc = skr_shade_rays(r, &pass, reinterpret_cast<const skr_ray *>(s.rays), m, aa, in, s.shade, stream);
			if(rc != SKR_OK) return rc;
			SKR_HIP(skr_launch_adaptive_sample(s, in, m, aa, samples, st));
		}
	}
	SKR_HIP(skr_launch_adaptive_resolve(s, pixels, d_rgb, d_rgbf, d_passes, d_var, st));
	return SKR_OK;
}

int skr_render_adaptive_var(skr_renderer *r, const skr_options *opt, const skr_adaptive *a, uint8_t *d_rgb, float *d_rgbf, uint32_t *d_passes, float *d_var,
							void *stream)
{
	return render_adaptive(r, "skr_render_adaptive_var", opt, a, d_rgb, d_rgbf, d_passes, d_var, stream);
}

int skr_render_adaptive(skr_renderer *r, const skr_options *opt, const skr_adaptive *a, uint8_t *d_rgb, float *d_rgbf, uint32_t *d_passes, void *stream)
{
	return render_adaptive(r, "skr_render_adaptive", opt, a, d_rgb, d_rgbf, d_passes, nullptr, stream); // (no variance image: an output of the three is needed)
}

int skr_render_adaptive_host(skr_renderer *r, const skr_options *opt, const skr_adaptive *a, uint8_t *h_rgb, float *h_rgbf, uint32_t *h_passes, float *kernel_ms)
{
	if(!r || !opt || !a || (!h_rgb && !h_rgbf && !h_passes))
	{
		skr_set_error("skr_render_adaptive_host: bad argument");
		return SKR_ERR_ARG;
	}
	int rc = check_adaptive(opt, a, "skr_render_adaptive_host"); // before anything is sized from width x height
	if(rc != SKR_OK) return rc;
	SKR_HIP(hipSetDevice(r->scene->device));
	const size_t pixels = (size_t) opt->width * opt->height;
	HostFrame f;
	rc = host_frame(r, pixels, true, f);
	if(rc != SKR_OK) return rc;
	uint8_t *d_rgb = h_rgb ? f.rgb : nullptr;
	float *d_rgbf = h_rgbf ? f.rgbf : nullptr;
	uint32_t *d_passes = h_passes ? f.passes : nullptr;
	return timed_host(r, [&] { return skr_render_adaptive(r, opt, a, d_rgb, d_rgbf, d_passes, nullptr); },
					  {{h_rgb, d_rgb, pixels * 3}, {h_rgbf, d_rgbf, pixels * 12}, {h_passes, d_passes, pixels * 4}}, kernel_ms);
}

// The two denoised host entries: the frame — `a` null: opt's own (the K-pass mean under progressive_passes), else the adaptive mean
// with its variance and pass counts — then its guides (the pixel centres' camera rays, traced) and the filter.  Only the pass counts
// wanted: the adaptive frame alone.  The entries have checked their arguments.
static int denoised_host(skr_renderer *r, const char *who, const skr_options *opt, const skr_adaptive *a, uint32_t iterations, uint8_t *h_rgb, float *h_rgbf,
						 uint32_t *h_passes, float *kernel_ms)
{
	if(r->scene->layout.lens_A > 0.0f)
	{ // a scene with a lens has no denoised frame (include/skr.h skr_scene_set_lens)
		skr_set_error("%s: a lens (--aperture) cannot be combined with the denoiser (its guides are the pinhole camera's first hits)", who);
		return SKR_ERR_UNSUPPORTED;
	}
	if(r->scene->layout.motion)
	{ // nor has a scene in motion (include/skr.h skr_scene_set_sphere_velocities)
		skr_set_error("%s: motion blur (sphere velocities under --shutter) cannot be combined with the denoiser (its guides are first hits of the scene at rest)", who);
		return SKR_ERR_UNSUPPORTED;
	}
	if(r->scene->layout.env_edge > 0)
	{ // nor has a scene with an environment (include/skr.h skr_scene_set_environment)
		skr_set_error("%s: an environment map (--envmap) cannot be combined with the denoiser (its guides hold one class for every miss: the filter would smear the backdrop)", who);
		return SKR_ERR_UNSUPPORTED;
	}
	if(r->scene->layout.textured)
	{ // nor has a scene with textures (include/skr.h skr_scene_add_texture)
		skr_set_error("%s: sphere textures (--scn-texture) cannot be combined with the denoiser (its guides hold one class per sphere: the filter would smear the pattern)", who);
		return SKR_ERR_UNSUPPORTED;
	}
	SKR_HIP(hipSetDevice(r->scene->device));
	const size_t n = (size_t) opt->width * opt->height;
	ScratchLayout L; // the frame, (adaptive) its variance and pass counts, the camera rays and guides, the filtered frame and its bytes
	const size_t o_frame = L.take(n * 12), o_var = a ? L.take(n * 4) : 0, o_passes = a ? L.take(n * 4) : 0, o_rays = L.take(n * sizeof(skr_ray)),
				 o_hits = L.take(n * sizeof(skr_hit)), o_out = L.take(n * 12), o_rgb = L.take(n * 3);
	const int rc = r->dnframe.grow(L.off);
	if(rc != SKR_OK) return rc;
	float *frame = r->dnframe.at<float>(o_frame), *var = a ? r->dnframe.at<float>(o_var) : nullptr, *out = r->dnframe.at<float>(o_out);
	uint32_t *passes = a ? r->dnframe.at<uint32_t>(o_passes) : nullptr;
	skr_ray *rays = r->dnframe.at<skr_ray>(o_rays);
	skr_hit *hits = r->dnframe.at<skr_hit>(o_hits);
	uint8_t *rgb = r->dnframe.at<uint8_t>(o_rgb);
	skr_options guide_opt = *opt;
	guide_opt.grid_size = 0; // the pixel centres
	const bool filtered = h_rgb || h_rgbf;
	return timed_host(r, [&]() -> int {
		int e = a ? skr_render_adaptive_var(r, opt, a, nullptr, frame, h_passes ? passes : nullptr, var, nullptr)
				  : skr_render_tiles(r, opt, (uint32_t) opt->height, 0, 1, nullptr, frame, nullptr);
		if(e == SKR_OK && filtered) e = skr_camera_rays(r, &guide_opt, 0, rays, nullptr);
		if(e == SKR_OK && filtered) e = skr_trace_rays(r, rays, (uint32_t) n, 0, hits, nullptr);
		if(e == SKR_OK && filtered)
			e = denoise(r, a ? "skr_denoise_var" : "skr_denoise", (uint32_t) opt->width, (uint32_t) opt->height, frame, hits, var, iterations, h_rgbf ? out : nullptr,
						h_rgb ? rgb : nullptr, nullptr);
		return e;
	}, {{h_rgb, rgb, n * 3}, {h_rgbf, out, n * 12}, {h_passes, passes, n * 4}}, kernel_ms);
}

int skr_render_denoised_host(skr_renderer *r, const skr_options *opt, uint32_t iterations, uint8_t *h_rgb, float *h_rgbf, float *kernel_ms)
{
	if(!r || !opt || (!h_rgb && !h_rgbf) || iterations > SKR_DENOISE_MAX_ITERATIONS)
	{
		skr_set_error("skr_render_denoised_host: bad argument");
		return SKR_ERR_ARG;
	}
	const int rc = check_options(opt); // before anything is sized from width x height
	return rc != SKR_OK ? rc : denoised_host(r, "skr_render_denoised_host", opt, nullptr, iterations, h_rgb, h_rgbf, nullptr, kernel_ms);
}

int skr_render_adaptive_denoised_host(skr_renderer *r, const skr_options *opt, const skr_adaptive *a, uint32_t iterations, uint8_t *h_rgb, float *h_rgbf,
									  uint32_t *h_passes, float *kernel_ms)
{
	if(!r || !opt || !a || (!h_rgb && !h_rgbf && !h_passes) || iterations > SKR_DENOISE_MAX_ITERATIONS)
	{
		skr_set_error("skr_render_adaptive_denoised_host: bad argument (no output, or iterations over %d)", SKR_DENOISE_MAX_ITERATIONS);
		return SKR_ERR_ARG;
	}
	const int rc = check_adaptive(opt, a, "skr_render_adaptive_denoised_host"); // before anything is sized from width x height
	return rc != SKR_OK ? rc : denoised_host(r, "skr_render_adaptive_denoised_host", opt, a, iterations, h_rgb, h_rgbf, h_passes, kernel_ms);
}

int skr_debug_eval(int op, const void *d_in, void *d_out, uint32_t n, void *stream)
{
	if(!d_in || !d_out || op < 0 || op > 26) return SKR_ERR_ARG;
	if(n == 0) return SKR_OK;
	SKR_HIP(skr_launch_debug(op, d_in, d_out, n, (hipStream_t) stream));
	return SKR_OK;
}

} // extern "C"

int skr_render_tile_list_owned(skr_renderer *r, const skr_options *opt, uint32_t tile_rows, const uint32_t *d_tiles, uint32_t n_slots, uint64_t table_id, uint8_t *d_rgb,
							   float *d_rgbf, void *stream)
{
	if(!d_tiles)
	{
		skr_set_error("skr_render_tile_list: no tile table");
		return SKR_ERR_ARG;
	}
	TileSel ts;
	ts.d_table = d_tiles;
	ts.n_slots = n_slots;
	ts.table_id = table_id;
	return render_impl(r, opt, tile_rows, ts, d_rgb, d_rgbf, stream);
}
