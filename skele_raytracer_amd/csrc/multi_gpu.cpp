// Native multi-GPU frame: the framebuffer sharded in interleaved row tiles over the GPUs of one node and gathered with
// ONE RCCL collective over xGMI (include/skr.h "multi-GPU").  The reference's parallel entry is one C++ process that fans
// the rows of a frame out over OpenMP threads (src/main.cpp:19-104, fan-out at :33, dispatch :402-410) and has no
// distributed path at all; this is its MI355X form, in the two shapes a caller needs:
//
//   skr_multi_*   ONE process drives N devices: a renderer, a stream and a worker thread per device, ncclCommInitAll,
//                 per frame one skr_render_tiles launch sequence per device and one grouped ncclAllGather of the u8 tile
//                 buffers (every rank renders straight into its slot of the gather buffer: no staging copy); the root
//                 de-interleaves on the device (a copy kernel) and owns the frame.  What `bin/raytracer --gpus N` uses.
//   skr_comm_*    one process PER device (torchrun, mpirun): the same frame step on a communicator made with
//                 ncclCommInitRank from an id the caller broadcasts by whatever transport it has.  What bench.py uses.
//
// Each has a serial step (the collective on the render stream) and a pipelined one (the collective on a stream of its own, two buffer
// sets).  All four are made of the same per-device parts: a Rank is what one device owns, render_rank its frame up to the collective,
// finish_rank what follows the collective.  Only the collective is the shape's own: one ncclAllGather per process (skr_comm) against
// one grouped call over every device (skr_multi).
//
// Tile t belongs to rank t mod G (cost is very non-uniform vertically); random numbers are keyed by the global pixel
// index, so the image does not depend on G.  RCCL is bound at run time (dlopen): libskr.so loads, and renders on one
// GPU, on a box without it, and inside a process that already carries an RCCL (PyTorch ships one) it uses that one.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <dlfcn.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "api_internal.h"

namespace {

// ---- RCCL, bound lazily ------------------------------------------------------------------------------------------
struct Rccl {
	bool ok = false;
	ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
	ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
	ncclResult_t (*CommInitAll)(ncclComm_t *, int, const int *) = nullptr;
	ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
	ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
	ncclResult_t (*GroupStart)() = nullptr;
	ncclResult_t (*GroupEnd)() = nullptr;
	const char *(*GetErrorString)(ncclResult_t) = nullptr;
};

Rccl &rccl()
{
	static Rccl r;
	static std::once_flag once;
	std::call_once(once, [] {
		// a copy already in the process (PyTorch's) first; then the ROCm installation's
		void *h = nullptr;
		if(dlsym(RTLD_DEFAULT, "ncclAllGather")) h = RTLD_DEFAULT;
		const char *names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
		for(int i = 0; !h && i < 3; i++) h = dlopen(names[i], RTLD_NOW | RTLD_LOCAL);
		if(!h) return;
		r.GetUniqueId = reinterpret_cast<decltype(r.GetUniqueId)>(dlsym(h, "ncclGetUniqueId"));
		r.CommInitRank = reinterpret_cast<decltype(r.CommInitRank)>(dlsym(h, "ncclCommInitRank"));
		r.CommInitAll = reinterpret_cast<decltype(r.CommInitAll)>(dlsym(h, "ncclCommInitAll"));
		r.CommDestroy = reinterpret_cast<decltype(r.CommDestroy)>(dlsym(h, "ncclCommDestroy"));
		r.AllGather = reinterpret_cast<decltype(r.AllGather)>(dlsym(h, "ncclAllGather"));
		r.GroupStart = reinterpret_cast<decltype(r.GroupStart)>(dlsym(h, "ncclGroupStart"));
		r.GroupEnd = reinterpret_cast<decltype(r.GroupEnd)>(dlsym(h, "ncclGroupEnd"));
		r.GetErrorString = reinterpret_cast<decltype(r.GetErrorString)>(dlsym(h, "ncclGetErrorString"));
		r.ok = r.GetUniqueId && r.CommInitRank && r.CommInitAll && r.CommDestroy && r.AllGather && r.GroupStart && r.GroupEnd && r.GetErrorString;
	});
	return r;
}

#define SKR_NCCL(call)                                                                                          \
	do                                                                                                          \
	{                                                                                                           \
		ncclResult_t e_ = (call);                                                                               \
		if(e_ != ncclSuccess)                                                                                   \
		{                                                                                                       \
			skr_set_error("%s failed: %s (%s:%d)", #call, rccl().GetErrorString(e_), __FILE__, __LINE__);      \
			return SKR_ERR_HIP;                                                                                 \
		}                                                                                                       \
	} while(0)

// ---- the partition (the one definition both shapes and the tests use) -------------------------------------------
uint32_t tiles_total(int32_t height, uint32_t tile_rows) { return ((uint32_t) height + tile_rows - 1) / tile_rows; }
uint32_t tiles_per_rank(int32_t height, uint32_t tile_rows, uint32_t world) { return (tiles_total(height, tile_rows) + world - 1) / world; }

// The tile -> (rank, slot) map: slot_of_tile[t] = rank * k_max + k; every rank has k_max = ceil(T / G) slots (the all-gather moves
// equal chunks).  Tiles differ in cost by an order of magnitude (sky rows: one ray per pixel; ground rows: a tree of up to
// 1 + N + N^2 rays under every pixel).  Two ways to deal them: blindly, tile t to rank t mod G (the tiles are a few rows high, so every
// rank gets a sample of the whole image), and by cost — every tile's own counted work (skr_tile_costs renders each tile once and reads
// the work counters, once per frame geometry), dealt longest-processing-time-first: most expensive tile first, each to the rank with
// the least work so far that still has a free slot.  Both are deterministic (integer counts of a bit-reproducible render, a stable
// sort, ties to the lower index), so every rank of a job computes the same map without talking to the others, and the image cannot
// change with the map: the RNG is keyed by the global pixel.  shard_rule() below says which one a frame step takes.
void shard_interleaved(uint32_t T, uint32_t world, uint32_t *slot_of_tile)
{
	const uint32_t k_max = (T + world - 1) / world;
	for(uint32_t t = 0; t < T; t++) slot_of_tile[t] = (t % world) * k_max + t / world;
}

void shard_lpt(const uint64_t *cost, uint32_t T, uint32_t world, uint32_t *slot_of_tile)
{
	const uint32_t k_max = (T + world - 1) / world;
	std::vector<uint32_t> order(T);
	for(uint32_t t = 0; t < T; t++) order[t] = t;
	std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return cost[a] > cost[b]; });
	std::vector<uint64_t> load(world, 0);
	std::vector<uint32_t> used(world, 0);
	for(uint32_t i = 0; i < T; i++)
	{
		const uint32_t t = order[i];
		uint32_t best = world;
		for(uint32_t r = 0; r < world; r++)
			if(used[r] < k_max && (best == world || load[r] < load[best])) best = r;
		slot_of_tile[t] = best; // (the rank for now)
		used[best]++;
		load[best] += cost[t];
	}
	// a rank's tiles sit in its slots in image order, as under the blind map: the kernels cut a launch into regions of consecutive
	// blocks, and dealing the slots in LPT order (all the expensive tiles first) cost 4 % of a share's time
	std::fill(used.begin(), used.end(), 0u);
	for(uint32_t t = 0; t < T; t++)
	{
		const uint32_t r = slot_of_tile[t];
		slot_of_tile[t] = r * k_max + used[r]++;
	}
}

// gathered: [world][k_max * tile_rows][row_bytes] (rank-major, what the all-gather leaves) -> frame[height][row_bytes]; row y of tile
// t = y / tile_rows lives in slot slot_of_tile[t].  One 16-byte word per thread where the rows allow it.
template <typename T>
__global__ __launch_bounds__(256) void skr_deinterleave_kernel(const T *gathered, T *frame, uint32_t height, uint32_t row_words, uint32_t tile_rows, const uint32_t *slot_of_tile)
{
	const uint64_t i = (uint64_t) blockIdx.x * 256u + threadIdx.x;
	if(i >= (uint64_t) height * row_words) return;
	const uint32_t y = (uint32_t) (i / row_words), x = (uint32_t) (i - (uint64_t) y * row_words);
	const uint32_t t = y / tile_rows;
	frame[i] = gathered[((uint64_t) slot_of_tile[t] * tile_rows + (y - t * tile_rows)) * row_words + x];
}

hipError_t launch_deinterleave(const uint8_t *gathered, uint8_t *frame, int32_t width, int32_t height, uint32_t tile_rows, const uint32_t *d_slot_of_tile, hipStream_t stream)
{
	const size_t row_bytes = (size_t) width * 3;
	if(row_bytes % 16 == 0 && (reinterpret_cast<uintptr_t>(gathered) | reinterpret_cast<uintptr_t>(frame)) % 16 == 0)
	{
		const uint32_t rw = (uint32_t) (row_bytes / 16);
		const uint64_t n = (uint64_t) height * rw;
		hipLaunchKernelGGL(skr_deinterleave_kernel<uint4>, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, stream, reinterpret_cast<const uint4 *>(gathered),
						   reinterpret_cast<uint4 *>(frame), (uint32_t) height, rw, tile_rows, d_slot_of_tile);
	}
	else
	{
		const uint64_t n = (uint64_t) height * row_bytes;
		hipLaunchKernelGGL(skr_deinterleave_kernel<uint8_t>, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, stream, gathered, frame, (uint32_t) height,
						   (uint32_t) row_bytes, tile_rows, d_slot_of_tile);
	}
	return hipGetLastError();
}

// What one rank's map and buffers of a frame are made for.  A frame whose key differs from the last frame's is a change of frame
// geometry: the map is rebuilt (and, unless SKR_SHARD=interleave, the tile costs probed again) and the buffers resized.
struct FrameKey {
	const skr_renderer *r = nullptr;
	int32_t width = 0, height = 0;
	float fov = 0;
	uint32_t tile_rows = 0, world = 0, rank = 0;
	int32_t monte_carlo = 0, gillum = 0, depth = 0;
	bool operator==(const FrameKey &o) const
	{
		return r == o.r && width == o.width && height == o.height && fov == o.fov && tile_rows == o.tile_rows && world == o.world && rank == o.rank &&
			   monte_carlo == o.monte_carlo && gillum == o.gillum && depth == o.depth;
	}
	bool operator!=(const FrameKey &o) const { return !(*this == o); }
};

// The map of one frame geometry on one device: host copy, and on the device the rank's own tile list (what skr_render_tile_list
// takes) and slot_of_tile (what the de-interleave takes).  Rebuilt when the geometry, the tree or the scene behind it changes.
struct ShardMap {
	FrameKey key;
	uint32_t T = 0, k_max = 0;
	std::vector<uint32_t> slot_of_tile;
	uint32_t *d_tiles = nullptr;        // k_max entries: the tiles of `rank` in slot order (0xFFFFFFFF: an empty slot)
	uint64_t generation = 0;            // names the contents of d_tiles: a new number, never 0, from next_generation() whenever the table is rebuilt
	uint32_t *d_slot_of_tile = nullptr; // T entries
};

// Which map a frame step takes.  Measured on the headline frame (tools/time_shard.py, profiles/r03_time_shard.txt): the blind map's
// slowest rank of 8 is 3 % above the mean, and LPT over the counted work does not beat it — ranks whose counted rays, hits and
// ray-sphere tests agree to 0.1 % still differ by 6 % in time when one of them holds the expensive tiles of ONE part of the image
// (what LPT deals first) and the other tiles from all over it.  So interleaving stays the rule, and the counted costs decide only
// whether it is safe: where the blind map's heaviest rank carries more than 1.10 of the mean cost (a frame whose expensive rows repeat
// with a period of G tiles; few tiles per rank), LPT takes over.  SKR_SHARD=interleave / lpt forces one or the other.
enum ShardRule { SHARD_AUTO, SHARD_INTERLEAVE, SHARD_LPT };
ShardRule shard_rule()
{
	const char *e = getenv("SKR_SHARD");
	if(e && !strcmp(e, "interleave")) return SHARD_INTERLEAVE;
	if(e && !strcmp(e, "lpt")) return SHARD_LPT;
	return SHARD_AUTO;
}

// true = the blind map leaves its heaviest rank above 1.10 of the mean cost
bool interleave_unbalanced(const uint64_t *cost, uint32_t T, uint32_t world)
{
	std::vector<uint64_t> load(world, 0);
	uint64_t total = 0;
	for(uint32_t t = 0; t < T; t++)
	{
		load[t % world] += cost[t];
		total += cost[t];
	}
	const uint64_t heaviest = *std::max_element(load.begin(), load.end());
	return (long double) heaviest * world * 100 > (long double) total * 110;
}

void shard_by_cost(const uint64_t *cost, uint32_t T, uint32_t world, ShardRule rule, uint32_t *slot_of_tile)
{
	if(rule == SHARD_LPT || (rule == SHARD_AUTO && interleave_unbalanced(cost, T, world))) shard_lpt(cost, T, world, slot_of_tile);
	else shard_interleaved(T, world, slot_of_tile);
}

int plan_map(skr_renderer *r, const skr_options *opt, uint32_t tile_rows, uint32_t world, uint32_t *slot_of_tile)
{
	const uint32_t T = tiles_total(opt->height, tile_rows);
	const ShardRule rule = shard_rule();
	if(world < 2 || rule == SHARD_INTERLEAVE)
	{
		shard_interleaved(T, world, slot_of_tile);
		return SKR_OK;
	}
	std::vector<uint64_t> cost(T);
	const int rc = skr_tile_costs(r, opt, tile_rows, cost.data());
	if(rc != SKR_OK) return rc;
	shard_by_cost(cost.data(), T, world, rule, slot_of_tile);
	return SKR_OK;
}

// One sequence for every map of the process: a renderer that kept its level-0 stage under one map's table (api.cpp render_pass) must not
// take another map's table at the same address for it.
uint64_t next_generation()
{
	static std::atomic<uint64_t> last{0};
	return ++last;
}

void free_map(ShardMap &m)
{
	if(m.d_tiles) (void) hipFree(m.d_tiles);
	if(m.d_slot_of_tile) (void) hipFree(m.d_slot_of_tile);
	m = ShardMap();
}

// `shared`: a map already computed for this geometry on another device of the same process (skr_multi): only uploaded here
int ensure_map(ShardMap &m, skr_renderer *r, const skr_options *opt, const FrameKey &key, const std::vector<uint32_t> *shared)
{
	if(m.d_tiles && m.key == key && (!shared || *shared == m.slot_of_tile)) return SKR_OK;
	free_map(m);
	m.key = key;
	m.T = tiles_total(key.height, key.tile_rows);
	m.k_max = tiles_per_rank(key.height, key.tile_rows, key.world);
	if(shared) m.slot_of_tile = *shared;
	else
	{
		m.slot_of_tile.assign(m.T, 0);
		const int rc = plan_map(r, opt, key.tile_rows, key.world, m.slot_of_tile.data());
		if(rc != SKR_OK) return rc;
	}
	std::vector<uint32_t> mine(m.k_max, 0xFFFFFFFFu);
	for(uint32_t t = 0; t < m.T; t++)
		if(m.slot_of_tile[t] / m.k_max == key.rank) mine[m.slot_of_tile[t] % m.k_max] = t;
	SKR_HIP(hipMalloc((void **) &m.d_tiles, (size_t) m.k_max * sizeof(uint32_t)));
	SKR_HIP(hipMalloc((void **) &m.d_slot_of_tile, (size_t) m.T * sizeof(uint32_t)));
	SKR_HIP(hipMemcpy(m.d_tiles, mine.data(), (size_t) m.k_max * sizeof(uint32_t), hipMemcpyHostToDevice));
	m.generation = next_generation();
	SKR_HIP(hipMemcpy(m.d_slot_of_tile, m.slot_of_tile.data(), (size_t) m.T * sizeof(uint32_t), hipMemcpyHostToDevice));
	return SKR_OK;
}

// one rank's buffers for one frame geometry
struct RankBuffers {
	FrameKey key;
	size_t chunk = 0;           // bytes one rank contributes: k_max * tile_rows * width * 3
	uint8_t *d_gather = nullptr; // [world][chunk]; this rank renders into slot `rank`
	uint8_t *d_frame = nullptr;  // root only: the de-interleaved frame
};

int size_buffers(RankBuffers &b, const FrameKey &key, bool root)
{
	if(b.d_gather && b.key == key) return SKR_OK;
	if(b.d_gather) SKR_HIP(hipFree(b.d_gather));
	if(b.d_frame) SKR_HIP(hipFree(b.d_frame));
	b.d_gather = b.d_frame = nullptr;
	b.key = key;
	b.chunk = (size_t) tiles_per_rank(key.height, key.tile_rows, key.world) * key.tile_rows * (size_t) key.width * 3;
	SKR_HIP(hipMalloc((void **) &b.d_gather, b.chunk * key.world));
	SKR_HIP(hipMemset(b.d_gather, 0, b.chunk * key.world)); // the padding rows of a last partial tile travel too
	if(root) SKR_HIP(hipMalloc((void **) &b.d_frame, (size_t) key.width * key.height * 3));
	return SKR_OK;
}

void free_buffers(RankBuffers &b)
{
	if(b.d_gather) (void) hipFree(b.d_gather);
	if(b.d_frame) (void) hipFree(b.d_frame);
	b = RankBuffers();
}

int check_frame_args(const skr_options *opt, uint32_t tile_rows)
{
	if(!opt || tile_rows == 0 || opt->width <= 0 || opt->height <= 0 || opt->width > 65536 || opt->height > 65536)
	{
		skr_set_error("multi-GPU frame: bad image size or tile_rows");
		return SKR_ERR_ARG;
	}
	return SKR_OK;
}

// A rank's share of a frame is eight short dependent kernels: two frames in flight on two streams fill each other's ramps and
// tails — 1/8 of the headline frame 0.258 -> 0.217 ms per frame, 1/4 0.454 -> 0.427, 1/2 0.836 -> 0.800 (tools/inflight.py); a whole frame
// through this step, with the de-interleave behind it, 1.570 -> 1.513 ms.  So a run of frames alternates between the renderer and a clone of
// it (a second set of tables: 1.7 GB for the headline frame); SKR_INFLIGHT=1 keeps it to one.
bool two_in_flight()
{
	if(const char *e = getenv("SKR_INFLIGHT")) return atoi(e) >= 2;
	return true;
}

constexpr int SERIAL = -1; // the buffer set of the serial frame step (the pipelined step's are 0 and 1)

// Everything one device owns for the frame steps, in either shape.  Complete from creation, but for the clone: the pipelined step makes
// it on the first odd frame of a run.
struct Rank {
	int device = 0, rank = 0, world = 1;
	ncclComm_t comm = nullptr; // nullptr: a world of one without RCCL
	skr_renderer *r = nullptr;
	bool owns_r = false;         // skr_multi makes its renderers, skr_comm borrows the caller's
	hipStream_t rs = nullptr;    // skr_multi: the render stream (skr_comm renders on the caller's stream) ...
	hipEvent_t called = nullptr; // ... skr_comm: the caller's stream as it stands at a call, which the clone's frames follow
	bool two = false;            // two_in_flight(), read at creation: buffer set 1 belongs to a clone of r on a stream of its own
	skr_renderer *r2 = nullptr;
	hipStream_t rs2 = nullptr;
	// the pipelined step: frame f's collective on cs while frame f + 1 is rendered into the other buffer set
	hipStream_t cs = nullptr;
	hipEvent_t rendered[2] = {nullptr, nullptr}, gathered[2] = {nullptr, nullptr};
	bool in_flight[2] = {false, false}; // a collective of set s was enqueued: gathered[s] marks its end
	RankBuffers buf, abuf[2];            // the serial step's buffer set; the pipelined step's two
	ShardMap map;                        // the tile -> rank map of the frame geometry last rendered

	FrameKey key(const skr_options *opt, uint32_t tile_rows) const
	{
		return {r, opt->width, opt->height, opt->fov, tile_rows, (uint32_t) world, (uint32_t) rank, opt->monte_carlo, opt->num_path_traces, opt->max_depth};
	}
	RankBuffers &buffers(int set) { return set == SERIAL ? buf : abuf[set]; }
};

// the streams and events of a rank, on its device (own_stream: skr_multi's, which render on a stream of their own)
int open_rank(Rank &k, bool own_stream)
{
	k.two = two_in_flight();
	SKR_HIP(hipSetDevice(k.device));
	if(own_stream) SKR_HIP(hipStreamCreateWithFlags(&k.rs, hipStreamNonBlocking));
	else SKR_HIP(hipEventCreateWithFlags(&k.called, hipEventDisableTiming));
	SKR_HIP(hipStreamCreateWithFlags(&k.cs, hipStreamNonBlocking));
	for(int s = 0; s < 2; s++)
	{
		SKR_HIP(hipEventCreateWithFlags(&k.rendered[s], hipEventDisableTiming));
		SKR_HIP(hipEventCreateWithFlags(&k.gathered[s], hipEventDisableTiming));
	}
	return SKR_OK;
}

void free_rank(Rank &k)
{
	(void) hipSetDevice(k.device);
	for(hipStream_t s : {k.rs, k.rs2, k.cs})
		if(s) (void) hipStreamSynchronize(s);
	free_buffers(k.buf);
	for(int s = 0; s < 2; s++)
	{
		free_buffers(k.abuf[s]);
		if(k.rendered[s]) (void) hipEventDestroy(k.rendered[s]);
		if(k.gathered[s]) (void) hipEventDestroy(k.gathered[s]);
	}
	free_map(k.map);
	if(k.called) (void) hipEventDestroy(k.called);
	for(hipStream_t s : {k.rs, k.rs2, k.cs})
		if(s) (void) hipStreamDestroy(s);
	if(k.r2) skr_renderer_destroy(k.r2);
	if(k.comm) (void) rccl().CommDestroy(k.comm);
	if(k.owns_r && k.r) skr_renderer_destroy(k.r);
}

// on the host, until the collective of every buffer set in flight on these ranks has ended
int wait_in_flight(Rank *ranks, int n)
{
	for(int i = 0; i < n; i++)
		for(int s = 0; s < 2; s++)
			if(ranks[i].in_flight[s]) SKR_HIP(hipEventSynchronize(ranks[i].gathered[s]));
	return SKR_OK;
}

// The pipelined steps' rule for a change of frame geometry: this frame resizes buffers and rebuilds the map that a collective still in
// flight may read, so every set in flight is waited for on the host first.  Both sets stay in flight: the previous frame's buffers are
// not the ones this frame resizes, and it is handed back as usual.
int settle(Rank *ranks, int n, const skr_options *opt, uint32_t tile_rows)
{
	for(int i = 0; i < n; i++)
		if((ranks[i].in_flight[0] || ranks[i].in_flight[1]) && ranks[i].map.key != ranks[i].key(opt, tile_rows)) return wait_in_flight(ranks, n);
	return SKR_OK;
}

// One device's frame up to the collective, into buffer set `set` (SERIAL, or 0 / 1 of the pipelined step): the renderer and the stream,
// the wait for the set's last collective, the buffers and the map, the render into this rank's slot of the gather buffer.  `rs`: the
// render stream (skr_comm: the caller's).  `shared`: device 0's map, for skr_multi's other devices to upload.  `start`: an event recorded
// just before the render (skr_multi's serial step, device 0).
//
// The order of a pipelined frame f on one device, set s = f mod 2:
//   - set 1 with two frames in flight: the clone renders, on rs2; under skr_comm rs2 first waits for `called`, recorded on the caller's
//     stream;
//   - the render stream waits for gathered[s] if set s is in flight (the collective of frame f - 2 read these buffers);
//   - the render, then rendered[s]; cs waits for rendered[s];
//   - the caller then enqueues on cs the all-gather, and finish_rank the de-interleave (root only) and gathered[s].
// The previous frame is handed back by each shape: skr_comm makes the caller's stream wait for gathered[prev], skr_multi waits for it on
// the host.  The serial step keeps the collective and the de-interleave on the render stream, with no events.
int render_rank(Rank &k, int set, const skr_options *opt, uint32_t tile_rows, hipStream_t rs, const std::vector<uint32_t> *shared, hipEvent_t start)
{
	SKR_HIP(hipSetDevice(k.device));
	skr_renderer *rr = k.r;
	if(set == 1 && k.two)
	{ // (the clone and its stream are made by this device's own thread, once)
		if(!k.r2)
		{
			const int rc = skr_renderer_clone(k.r, &k.r2);
			if(rc != SKR_OK) return rc;
			SKR_HIP(hipStreamCreateWithFlags(&k.rs2, hipStreamNonBlocking));
		}
		skr_copy_switches(k.r2, k.r);
		if(k.called)
		{
			SKR_HIP(hipEventRecord(k.called, rs));
			SKR_HIP(hipStreamWaitEvent(k.rs2, k.called, 0));
		}
		rs = k.rs2;
		rr = k.r2;
	}
	if(set != SERIAL && k.in_flight[set]) SKR_HIP(hipStreamWaitEvent(rs, k.gathered[set], 0));
	RankBuffers &b = k.buffers(set);
	const FrameKey key = k.key(opt, tile_rows);
	int rc = size_buffers(b, key, k.rank == 0);
	if(rc != SKR_OK) return rc;
	rc = ensure_map(k.map, k.r, opt, key, shared);
	if(rc != SKR_OK) return rc;
	if(start) SKR_HIP(hipEventRecord(start, rs));
	rc = skr_render_tile_list_owned(rr, opt, tile_rows, k.map.d_tiles, k.map.k_max, k.map.generation, b.d_gather + (size_t) k.rank * b.chunk, nullptr, rs);
	if(rc != SKR_OK) return rc;
	if(set != SERIAL)
	{
		SKR_HIP(hipEventRecord(k.rendered[set], rs));
		SKR_HIP(hipStreamWaitEvent(k.cs, k.rendered[set], 0));
	}
	return SKR_OK;
}

// this rank's slot of the set's gather buffer to every rank, in place (slot `rank` is the send buffer)
ncclResult_t all_gather(Rank &k, int set, hipStream_t on)
{
	RankBuffers &b = k.buffers(set);
	return rccl().AllGather(b.d_gather + (size_t) k.rank * b.chunk, b.d_gather, b.chunk, ncclUint8, k.comm, on);
}

// behind the all-gather on `on`: the root's de-interleave, then (pipelined) gathered[set], what the next user of the set waits for
int finish_rank(Rank &k, int set, hipStream_t on)
{
	RankBuffers &b = k.buffers(set);
	if(k.rank == 0) SKR_HIP(launch_deinterleave(b.d_gather, b.d_frame, b.key.width, b.key.height, b.key.tile_rows, k.map.d_slot_of_tile, on));
	if(set != SERIAL)
	{
		SKR_HIP(hipEventRecord(k.gathered[set], on));
		k.in_flight[set] = true;
	}
	return SKR_OK;
}

// skr_comm's collective: one all-gather per process (none in a world of one without RCCL), then finish_rank
int comm_collect(Rank &k, int set, hipStream_t on)
{
	if(k.comm) SKR_NCCL(all_gather(k, set, on));
	return finish_rank(k, set, on);
}

} // namespace

// =====================================================================================================================
// one process per device
// =====================================================================================================================
struct skr_comm {
	Rank k; // the renderer is the caller's
	uint64_t async_frames = 0;
};

extern "C" {

int skr_rccl_available(void) { return rccl().ok ? 1 : 0; }

int skr_comm_unique_id(uint8_t id[SKR_COMM_ID_BYTES])
{
	static_assert(SKR_COMM_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "include/skr.h carries RCCL's id size");
	if(!id) return SKR_ERR_ARG;
	if(!rccl().ok)
	{
		skr_set_error("RCCL (librccl.so.1) is not loadable in this process");
		return SKR_ERR_UNSUPPORTED;
	}
	ncclUniqueId u;
	SKR_NCCL(rccl().GetUniqueId(&u));
	memcpy(id, u.internal, SKR_COMM_ID_BYTES);
	return SKR_OK;
}

int skr_comm_create(skr_renderer *r, int device, const uint8_t id[SKR_COMM_ID_BYTES], int rank, int world, skr_comm **out)
{
	if(!r || !out || world < 1 || rank < 0 || rank >= world || (world > 1 && !id))
	{
		skr_set_error("skr_comm_create: bad argument");
		return SKR_ERR_ARG;
	}
	*out = nullptr;
	const bool with_rccl = world > 1 || id; // (a world of one still goes through RCCL when the caller hands an id: how the path is exercised on a one-GPU box)
	if(with_rccl && !rccl().ok)
	{
		skr_set_error("RCCL (librccl.so.1) is not loadable in this process");
		return SKR_ERR_UNSUPPORTED;
	}
	skr_comm *c = new skr_comm();
	Rank &k = c->k;
	k.r = r;
	k.device = device;
	k.rank = rank;
	k.world = world;
	int rc = open_rank(k, false);
	if(rc == SKR_OK && with_rccl)
	{
		ncclUniqueId u;
		memcpy(u.internal, id, SKR_COMM_ID_BYTES);
		const ncclResult_t ne = rccl().CommInitRank(&k.comm, world, u, rank);
		if(ne != ncclSuccess)
		{
			skr_set_error("ncclCommInitRank(rank %d of %d, device %d) failed: %s", rank, world, device, rccl().GetErrorString(ne));
			k.comm = nullptr;
			rc = SKR_ERR_HIP;
		}
	}
	if(rc != SKR_OK)
	{
		skr_comm_destroy(c);
		return rc;
	}
	*out = c;
	return SKR_OK;
}

void skr_comm_destroy(skr_comm *c)
{
	if(!c) return;
	free_rank(c->k);
	delete c;
}

// This rank's tiles, the collective, and (rank 0) the de-interleave, all enqueued on `stream`.  *d_frame (rank 0) points
// at the finished W x H x 3 frame in device memory once the stream has drained; other ranks get NULL.
int skr_comm_render_frame(skr_comm *c, const skr_options *opt, uint32_t tile_rows, uint8_t **d_frame, void *stream)
{
	if(!c) return SKR_ERR_ARG;
	int rc = check_frame_args(opt, tile_rows);
	if(rc != SKR_OK) return rc;
	rc = render_rank(c->k, SERIAL, opt, tile_rows, (hipStream_t) stream, nullptr, nullptr);
	if(rc != SKR_OK) return rc;
	rc = comm_collect(c->k, SERIAL, (hipStream_t) stream);
	if(rc != SKR_OK) return rc;
	if(d_frame) *d_frame = c->k.rank == 0 ? c->k.buf.d_frame : nullptr;
	return SKR_OK;
}

// The same frame step with the collective off the render stream: frame f's all-gather and de-interleave run on a stream of the
// communicator's own while frame f + 1 is rendered into the other of two buffer sets — on 8 GPUs the collective
// is a third of a 0.3 ms share, and nothing in the next frame depends on it.  The frames of a run also
// alternate between two renderers on two streams (two_in_flight above): throughput of a run, not the latency of a frame.  *d_prev_frame (rank 0): the frame of the
// PREVIOUS call, complete in `stream` order after this call (NULL on the first call and on the other ranks).
int skr_comm_render_frame_async(skr_comm *c, const skr_options *opt, uint32_t tile_rows, uint8_t **d_prev_frame, void *stream)
{
	if(!c) return SKR_ERR_ARG;
	int rc = check_frame_args(opt, tile_rows);
	if(rc != SKR_OK) return rc;
	Rank &k = c->k;
	const int s = (int) (c->async_frames & 1u), prev = s ^ 1;
	rc = settle(&k, 1, opt, tile_rows);
	if(rc != SKR_OK) return rc;
	rc = render_rank(k, s, opt, tile_rows, (hipStream_t) stream, nullptr, nullptr);
	if(rc != SKR_OK) return rc;
	rc = comm_collect(k, s, k.cs);
	if(rc != SKR_OK) return rc;
	c->async_frames++;
	if(d_prev_frame)
	{ // the previous frame: whatever `stream` does from here on sees it whole (a caller that passes NULL does not look, and saves the wait)
		*d_prev_frame = nullptr;
		if(k.in_flight[prev])
		{
			SKR_HIP(hipStreamWaitEvent((hipStream_t) stream, k.gathered[prev], 0));
			if(k.rank == 0) *d_prev_frame = k.abuf[prev].d_frame;
		}
	}
	return SKR_OK;
}

// Ends a run of skr_comm_render_frame_async calls: `stream` waits for the last frame's collective; *d_frame (rank 0) = that frame.
int skr_comm_flush(skr_comm *c, uint8_t **d_frame, void *stream)
{
	if(!c) return SKR_ERR_ARG;
	if(d_frame) *d_frame = nullptr;
	if(c->async_frames == 0) return SKR_OK;
	Rank &k = c->k;
	SKR_HIP(hipSetDevice(k.device));
	for(int s = 0; s < 2; s++)
		if(k.in_flight[s]) SKR_HIP(hipStreamWaitEvent((hipStream_t) stream, k.gathered[s], 0));
	if(d_frame && k.rank == 0) *d_frame = k.abuf[(c->async_frames - 1) & 1u].d_frame;
	return SKR_OK;
}

// Rank 0: waits for `stream` and copies the frame of the last skr_comm_render_frame to host memory (W*H*3 bytes).
int skr_comm_frame_to_host(skr_comm *c, uint8_t *h_rgb, void *stream)
{
	if(!c || !h_rgb || c->k.rank != 0 || !c->k.buf.d_frame)
	{
		skr_set_error("skr_comm_frame_to_host: rank 0 only, after skr_comm_render_frame");
		return SKR_ERR_ARG;
	}
	const RankBuffers &b = c->k.buf;
	SKR_HIP(hipSetDevice(c->k.device));
	SKR_HIP(hipStreamSynchronize((hipStream_t) stream));
	SKR_HIP(hipMemcpy(h_rgb, b.d_frame, (size_t) b.key.width * b.key.height * 3, hipMemcpyDeviceToHost));
	return SKR_OK;
}

} // extern "C"

// =====================================================================================================================
// one process, N devices
// =====================================================================================================================
struct skr_multi {
	int n = 0;
	std::vector<Rank> ranks; // device 0's map is computed there and uploaded to every other device
	uint64_t async_frames = 0;
	hipEvent_t e0 = nullptr, e1 = nullptr; // root stream: frame time
	// one worker thread per device (a single thread would enqueue 8 devices' launch sequences one after the other)
	std::vector<std::thread> workers;
	std::mutex mu;
	std::condition_variable cv_go, cv_done;
	uint64_t generation = 0;
	int pending = 0;
	bool quit = false;
	struct Job {
		const skr_options *opt;
		uint32_t tile_rows;
		int set; // the buffer set every device renders into
	} job = {nullptr, 0, SERIAL}; // what the workers are woken with
	std::vector<int> status;
	std::vector<std::string> errors;
};

namespace {

// what one device does for a frame: its tiles into its slot of its gather buffer (the collective follows, grouped, from the caller)
int multi_render_rank(skr_multi *m, int i, const skr_multi::Job &job)
{
	Rank &k = m->ranks[i];
	return render_rank(k, job.set, job.opt, job.tile_rows, k.rs, i != 0 ? &m->ranks[0].map.slot_of_tile : nullptr, i == 0 && job.set == SERIAL ? m->e0 : nullptr);
}

// every device renders its tiles of one frame (the calling thread drives device 0, the workers the others); returns when all are enqueued
int multi_render_all(skr_multi *m, const skr_options *opt, uint32_t tile_rows, int set)
{
	Rank &k0 = m->ranks[0];
	SKR_HIP(hipSetDevice(k0.device));
	int rc = ensure_map(k0.map, k0.r, opt, k0.key(opt, tile_rows), nullptr); // (before the workers upload it)
	if(rc != SKR_OK) return rc;
	{
		std::lock_guard<std::mutex> lk(m->mu);
		m->job = {opt, tile_rows, set};
		m->pending = m->n - 1;
		m->generation++;
	}
	m->cv_go.notify_all();
	m->status[0] = multi_render_rank(m, 0, m->job);
	if(m->status[0] != SKR_OK) m->errors[0] = skr_last_error();
	{
		std::unique_lock<std::mutex> lk(m->mu);
		m->cv_done.wait(lk, [&] { return m->pending == 0; });
	}
	for(int i = 0; i < m->n; i++)
		if(m->status[i] != SKR_OK)
		{
			skr_set_error("device %d: %s", m->ranks[i].device, m->errors[i].c_str());
			return m->status[i];
		}
	return SKR_OK;
}

// one grouped all-gather of every device's chunk, each on its device's collective stream (the render stream in the serial step), then
// the rest of the frame on every device
int multi_collect(skr_multi *m, int set)
{
	auto on = [set](const Rank &k) { return set == SERIAL ? k.rs : k.cs; };
	if(m->ranks[0].comm)
	{
		SKR_NCCL(rccl().GroupStart());
		for(Rank &k : m->ranks)
		{
			const ncclResult_t ne = all_gather(k, set, on(k));
			if(ne != ncclSuccess)
			{
				(void) rccl().GroupEnd();
				skr_set_error("ncclAllGather(rank %d) failed: %s", k.rank, rccl().GetErrorString(ne));
				return SKR_ERR_HIP;
			}
		}
		SKR_NCCL(rccl().GroupEnd());
	}
	for(Rank &k : m->ranks)
	{
		SKR_HIP(hipSetDevice(k.device));
		const int rc = finish_rank(k, set, on(k));
		if(rc != SKR_OK) return rc;
	}
	return SKR_OK;
}

void worker_main(skr_multi *m, int i)
{
	uint64_t seen = 0;
	for(;;)
	{
		skr_multi::Job job;
		{
			std::unique_lock<std::mutex> lk(m->mu);
			m->cv_go.wait(lk, [&] { return m->quit || m->generation != seen; });
			if(m->quit) return;
			seen = m->generation;
			job = m->job;
		}
		const int rc = multi_render_rank(m, i, job);
		{
			std::lock_guard<std::mutex> lk(m->mu);
			m->status[i] = rc;
			if(rc != SKR_OK) m->errors[i] = skr_last_error(); // (the error text is thread-local)
			if(--m->pending == 0) m->cv_done.notify_all();
		}
	}
}

} // namespace

extern "C" {

int skr_multi_create(const skr_scene *scene, int n_devices, const int *devices, skr_multi **out)
{
	if(!scene || !out || n_devices < 1)
	{
		skr_set_error("skr_multi_create: bad argument");
		return SKR_ERR_ARG;
	}
	*out = nullptr;
	int have = 0;
	if(hipGetDeviceCount(&have) != hipSuccess || have < n_devices)
	{
		skr_set_error("%d device(s) asked for, %d visible; libskr has no CPU fallback", n_devices, have);
		return SKR_ERR_NO_DEVICE;
	}
	if(n_devices > 1 && !rccl().ok)
	{
		skr_set_error("RCCL (librccl.so.1) is not loadable in this process");
		return SKR_ERR_UNSUPPORTED;
	}
	skr_multi *m = new skr_multi();
	m->n = n_devices;
	m->ranks.resize(n_devices);
	m->status.assign(n_devices, SKR_OK);
	m->errors.resize(n_devices);
	std::vector<int> ids(n_devices);
	int rc = SKR_OK;
	for(int i = 0; i < n_devices && rc == SKR_OK; i++)
	{ // the scene is uploaded to every device from the host: <= 0.5 MB, no collective needed
		Rank &k = m->ranks[i];
		k.device = ids[i] = devices ? devices[i] : i;
		k.rank = i;
		k.world = n_devices;
		k.owns_r = true;
		rc = skr_renderer_create(scene, k.device, &k.r);
		if(rc == SKR_OK) rc = open_rank(k, true);
	}
	if(rc == SKR_OK && rccl().ok)
	{ // (one device too, when RCCL is there: the same frame step, and the path that a one-GPU box can test)
		std::vector<ncclComm_t> comms(n_devices, nullptr);
		const ncclResult_t ne = rccl().CommInitAll(comms.data(), n_devices, ids.data());
		if(ne != ncclSuccess)
		{
			skr_set_error("ncclCommInitAll(%d devices) failed: %s", n_devices, rccl().GetErrorString(ne));
			rc = SKR_ERR_HIP;
		}
		else
			for(int i = 0; i < n_devices; i++) m->ranks[i].comm = comms[i];
	}
	if(rc == SKR_OK && (hipSetDevice(ids[0]) != hipSuccess || hipEventCreate(&m->e0) != hipSuccess || hipEventCreate(&m->e1) != hipSuccess))
	{
		skr_set_error("event creation failed");
		rc = SKR_ERR_HIP;
	}
	if(rc != SKR_OK)
	{
		skr_multi_destroy(m);
		return rc;
	}
	for(int i = 1; i < n_devices; i++) m->workers.emplace_back(worker_main, m, i); // device 0 is driven by the calling thread
	*out = m;
	return SKR_OK;
}

void skr_multi_destroy(skr_multi *m)
{
	if(!m) return;
	{
		std::lock_guard<std::mutex> lk(m->mu);
		m->quit = true;
	}
	m->cv_go.notify_all();
	for(std::thread &t : m->workers) t.join();
	for(Rank &k : m->ranks) free_rank(k);
	if(m->e0) (void) hipEventDestroy(m->e0);
	if(m->e1) (void) hipEventDestroy(m->e1);
	delete m;
}

int skr_multi_device_count(const skr_multi *m) { return m ? m->n : 0; }

skr_renderer *skr_multi_renderer(skr_multi *m, int i) { return (m && i >= 0 && i < m->n) ? m->ranks[i].r : nullptr; }

// The whole frame: every device its tiles, one grouped all-gather, the root's de-interleave; synchronous.  *d_frame is the
// W x H x 3 frame in device 0's memory (owned by m, valid until the next call); frame_ms = first launch to de-interleaved
// frame on the root's stream.
int skr_multi_render_frame(skr_multi *m, const skr_options *opt, uint32_t tile_rows, uint8_t **d_frame, float *frame_ms)
{
	if(!m) return SKR_ERR_ARG;
	int rc = check_frame_args(opt, tile_rows);
	if(rc != SKR_OK) return rc;
	rc = multi_render_all(m, opt, tile_rows, SERIAL);
	if(rc != SKR_OK) return rc;
	rc = multi_collect(m, SERIAL); // every rank's chunk to every rank (the root is the one that uses it), each on its rank's stream behind its kernels
	if(rc != SKR_OK) return rc;
	const Rank &k0 = m->ranks[0];
	SKR_HIP(hipSetDevice(k0.device));
	SKR_HIP(hipEventRecord(m->e1, k0.rs));
	for(int i = m->n - 1; i >= 0; i--)
	{
		SKR_HIP(hipSetDevice(m->ranks[i].device));
		SKR_HIP(hipStreamSynchronize(m->ranks[i].rs));
	}
	if(frame_ms) SKR_HIP(hipEventElapsedTime(frame_ms, m->e0, m->e1));
	if(d_frame) *d_frame = k0.buf.d_frame;
	return SKR_OK;
}

// The pipelined form (what skr_comm_render_frame_async is to skr_comm_render_frame): frame f's all-gather and de-interleave go to a
// second stream per device, behind an event the render stream records, while the render streams go on to frame f + 1 in the other of
// two buffer sets.  Returns as soon as frame f is enqueued; *d_prev_frame = the frame of the PREVIOUS call, complete (its collective
// is waited for on the host — it ran while this call's kernels were being enqueued), or NULL on the first call.
int skr_multi_render_frame_async(skr_multi *m, const skr_options *opt, uint32_t tile_rows, uint8_t **d_prev_frame)
{
	if(!m) return SKR_ERR_ARG;
	int rc = check_frame_args(opt, tile_rows);
	if(rc != SKR_OK) return rc;
	const int s = (int) (m->async_frames & 1u), prev = s ^ 1;
	rc = settle(m->ranks.data(), m->n, opt, tile_rows);
	if(rc != SKR_OK) return rc;
	rc = multi_render_all(m, opt, tile_rows, s);
	if(rc != SKR_OK) return rc;
	rc = multi_collect(m, s);
	if(rc != SKR_OK) return rc;
	m->async_frames++;
	if(d_prev_frame)
	{
		const Rank &k0 = m->ranks[0];
		*d_prev_frame = nullptr;
		if(k0.in_flight[prev])
		{
			SKR_HIP(hipEventSynchronize(k0.gathered[prev]));
			*d_prev_frame = k0.abuf[prev].d_frame;
		}
	}
	return SKR_OK;
}

// Ends a run of skr_multi_render_frame_async calls: waits for everything in flight; *d_frame = the last frame.
int skr_multi_flush(skr_multi *m, uint8_t **d_frame)
{
	if(!m) return SKR_ERR_ARG;
	if(d_frame) *d_frame = nullptr;
	if(m->async_frames == 0) return SKR_OK;
	const int rc = wait_in_flight(m->ranks.data(), m->n);
	if(rc != SKR_OK) return rc;
	if(d_frame) *d_frame = m->ranks[0].abuf[(m->async_frames - 1) & 1u].d_frame;
	return SKR_OK;
}

int skr_multi_render_frame_host(skr_multi *m, const skr_options *opt, uint32_t tile_rows, uint8_t *h_rgb, float *frame_ms)
{
	if(!h_rgb) return SKR_ERR_ARG;
	uint8_t *d = nullptr;
	const int rc = skr_multi_render_frame(m, opt, tile_rows, &d, frame_ms);
	if(rc != SKR_OK) return rc;
	SKR_HIP(hipMemcpy(h_rgb, d, (size_t) opt->width * opt->height * 3, hipMemcpyDeviceToHost));
	return SKR_OK;
}

// The partition, for callers and tests: tiles per rank (padded) and the (rank, slot) of a row's tile.
uint32_t skr_shard_tiles_per_rank(int32_t height, uint32_t tile_rows, uint32_t world)
{
	return (height > 0 && tile_rows && world) ? tiles_per_rank(height, tile_rows, world) : 0;
}

// The cost-aware map (longest processing time first; see shard_lpt above) for callers and tests: cost[t] per tile, any unit;
// slot_of_tile[t] = rank * k_max + slot.
int skr_shard_lpt(const uint64_t *cost, uint32_t n_tiles, uint32_t world, uint32_t *slot_of_tile)
{
	if(!cost || !slot_of_tile || !n_tiles || !world) return SKR_ERR_ARG;
	shard_lpt(cost, n_tiles, world, slot_of_tile);
	return SKR_OK;
}

// The map a frame step of `world` ranks uses for this renderer's scene and these options (plan_map above).  Synchronous; slot_of_tile has ceil(height / tile_rows) entries.
int skr_shard_plan(skr_renderer *r, const skr_options *opt, uint32_t tile_rows, uint32_t world, uint32_t *slot_of_tile)
{
	if(!r || !slot_of_tile || !world) return SKR_ERR_ARG;
	int rc = check_frame_args(opt, tile_rows);
	if(rc != SKR_OK) return rc;
	return plan_map(r, opt, tile_rows, world, slot_of_tile);
}

// The rule of the frame steps on given costs (tests): the blind map unless it leaves its heaviest rank above 1.10 of the mean cost.
int skr_shard_by_cost(const uint64_t *cost, uint32_t n_tiles, uint32_t world, uint32_t *slot_of_tile)
{
	if(!cost || !slot_of_tile || !n_tiles || !world) return SKR_ERR_ARG;
	shard_by_cost(cost, n_tiles, world, SHARD_AUTO, slot_of_tile);
	return SKR_OK;
}

// Host-side de-interleave of a rank-major gathered buffer under a map (what the device kernel does), for tests.
int skr_shard_deinterleave_map_host(const uint8_t *gathered, uint8_t *frame, int32_t width, int32_t height, uint32_t tile_rows, const uint32_t *slot_of_tile)
{
	if(!gathered || !frame || !slot_of_tile || width <= 0 || height <= 0 || !tile_rows) return SKR_ERR_ARG;
	const size_t row = (size_t) width * 3;
	for(uint32_t y = 0; y < (uint32_t) height; y++)
	{
		const uint32_t t = y / tile_rows;
		memcpy(frame + (size_t) y * row, gathered + ((size_t) slot_of_tile[t] * tile_rows + (y - t * tile_rows)) * row, row);
	}
	return SKR_OK;
}

// Host-side de-interleave of a rank-major gathered buffer (what the device kernel does), for tests and for callers that
// gathered by other means.
int skr_shard_deinterleave_host(const uint8_t *gathered, uint8_t *frame, int32_t width, int32_t height, uint32_t tile_rows, uint32_t world)
{
	if(!gathered || !frame || width <= 0 || height <= 0 || !tile_rows || !world) return SKR_ERR_ARG;
	const size_t row = (size_t) width * 3, k_max = tiles_per_rank(height, tile_rows, world);
	for(uint32_t y = 0; y < (uint32_t) height; y++)
	{
		const uint32_t t = y / tile_rows, rank = t % world, k = t / world;
		memcpy(frame + (size_t) y * row, gathered + ((size_t) rank * k_max * tile_rows + (size_t) k * tile_rows + (y - t * tile_rows)) * row, row);
	}
	return SKR_OK;
}

} // extern "C"
