// abg_sg.hip -- SimpleGraph's constrained path searches on the GPU and the abg_sg_* entry points (include/abyss_amd.h).
//
// A search is serial by contract (its visit count and which 201 paths it keeps depend on the order of the depth-first search), so
// the parallelism is across searches: a lane a search.  sg_search_kernel is one flat loop: a lane without a search takes the next
// index from an atomic counter, a lane with one runs abg::sg_step (abg_sg.h) once.  A search of 100,000 dependent steps therefore
// holds one lane, not its wave: the other 63 keep taking new searches beside it.  Frames live in global memory, frame d of lane L
// at stack[d * lanes + L], so a wave's lanes at one depth touch consecutive 16-byte slots.  A recorded path is appended to the
// call's arena by one atomic reservation as {search, length, vertices}; a lane's reservations ascend, so reading the arena in
// address order gives every search its paths in discovery order.  A search that outgrows the stack depth or finds the arena full
// is flagged, as is one with more constraints than the satisfied mask holds.  abg_sg_search launches those that found the arena
// full again, fewer at a time, and runs what is still flagged on the host with the same abg_sg.h body: a limit costs time, never a
// result.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/abyss_amd.h"
#include "abg_sg.h"
#include "abg_stage.h"

namespace st = abg::stage;

namespace {

struct DevStack {
	uint4* base; // this lane's column: frame d at base[d * stride]
	uint32_t stride, depth_cap;
	__device__ uint32_t cap() const { return depth_cap; }
	__device__ void store(uint32_t i, const abg::SGFrame& f) { base[(uint64_t)i * stride] = make_uint4(f.u, f.cur, (uint32_t)f.dist, (uint32_t)f.csat); }
	__device__ abg::SGFrame load(uint32_t i) const
	{
		const uint4 x = base[(uint64_t)i * stride];
		return abg::SGFrame{ x.x, x.y, (int32_t)x.z, (int32_t)x.w };
	}
	__device__ uint32_t vertex(uint32_t i) const { return base[(uint64_t)i * stride].x; }
};

struct DevSink {
	uint32_t* arena;
	unsigned long long* cursor;
	uint64_t cap; // words
	uint32_t search;
	__device__ bool emit(const DevStack& st, uint32_t depth, uint32_t top, uint32_t v)
	{
		const uint64_t len = (uint64_t)depth + 1;
		const uint64_t off = atomicAdd(cursor, (unsigned long long)(len + 2));
		if (off + len + 2 > cap) { atomicMin(cursor + 1, (unsigned long long)off); return false; } // cursor[1]: where the records end
		uint32_t* p = arena + off;
		p[0] = search;
		p[1] = (uint32_t)len;
		p += 2;
		for (uint32_t i = 1; i < depth; ++i) *p++ = st.vertex(i);
		if (depth > 0) *p++ = top;
		*p = v;
		return true;
	}
};

// counters[0]: the next search, counters[1]: steps taken while fewer than half the wave's lanes held a search, counters[2]: steps
__global__ __launch_bounds__(64) void sg_search_kernel(abg::SGGraph g, const abg::SGJob* __restrict__ jobs, const uint32_t* __restrict__ cv,
    const int32_t* __restrict__ cb, uint32_t njobs, uint32_t max_cost, uint32_t max_paths, uint4* __restrict__ stack, uint32_t depth_cap,
    uint32_t* __restrict__ arena, uint64_t arena_words, unsigned long long* cursor, unsigned long long* counters,
    uint32_t* __restrict__ visited, uint32_t* __restrict__ status, int count_busy)
{
	const uint32_t lanes = gridDim.x * blockDim.x;
	const uint32_t lane = blockIdx.x * blockDim.x + threadIdx.x;
	DevStack st{ stack + lane, lanes, depth_cap };
	DevSink sink{ arena, cursor, arena_words, 0 };
	abg::SGState<abg::SGSat64> s;
	abg::SGJob job{ 0, 0, 0, 0 };
	bool have = false;
	unsigned long long steps = 0, thin = 0;
	for (;;) {
		if (!have) {
			const unsigned long long i = atomicAdd(&counters[0], 1ull);
			if (i >= njobs) break;
			sink.search = (uint32_t)i;
			job = jobs[i];
			abg::sg_begin(g, job.origin, s);
			have = true;
		}
		if (count_busy) {
			const int busy = __popcll(__ballot(1));
			if (threadIdx.x == (unsigned)(__ffsll((long long)__ballot(1)) - 1)) { ++steps; if (busy < 32) ++thin; }
		}
		const int r = abg::sg_step(g, cv + job.coff, cb + job.coff, job.nc, max_cost, max_paths, s, st, sink);
		if (r != abg::SG_RUNNING) {
			visited[sink.search] = s.visited;
			status[sink.search] = (uint32_t)r;
			have = false;
		}
	}
	if (count_busy && steps) { atomicAdd(&counters[1], thin); atomicAdd(&counters[2], steps); }
}

} // namespace

struct abg_sg {
	int device = 0;
	hipStream_t stream = nullptr;
	// the graph on both sides
	std::vector<uint32_t> voff, vlen, etgt;
	std::vector<int32_t> edist;
	uint32_t* d_voff = nullptr; uint32_t* d_vlen = nullptr; uint32_t* d_etgt = nullptr; int32_t* d_edist = nullptr;
	bool have_graph = false;
	// limits (the frame stack of a launch is lanes * stack_depth * 16 bytes: 256 MiB at these defaults)
	uint32_t stack_depth = 512, max_constraints = abg::SG_MAX_CONSTRAINTS, max_lanes = 32768;
	uint64_t arena_words = 1ull << 24, batch = 1ull << 20;
	void* din = nullptr; size_t in_cap = 0;
	void* dstack = nullptr; size_t stack_cap = 0;
	void* darena = nullptr; size_t arena_cap = 0;
	void* dout = nullptr; size_t out_cap = 0;
	// the paths of the last call
	std::vector<uint64_t> path_off;
	std::vector<uint32_t> nodes;
	int profiling = 0; // 1: events around the launches; 2: the kernel also counts its wave steps
	st::Profile prof;
	uint64_t thin_steps = 0, all_steps = 0, redone = 0;
	std::string error;
	void free_graph()
	{
		if (d_voff) (void)hipFree(d_voff);
		if (d_vlen) (void)hipFree(d_vlen);
		if (d_etgt) (void)hipFree(d_etgt);
		if (d_edist) (void)hipFree(d_edist);
		d_voff = d_vlen = d_etgt = nullptr;
		d_edist = nullptr;
		have_graph = false;
	}
	~abg_sg()
	{
		(void)hipSetDevice(device);
		if (stream) (void)hipStreamSynchronize(stream);
		prof.drop();
		free_graph();
		if (din) (void)hipFree(din);
		if (dstack) (void)hipFree(dstack);
		if (darena) (void)hipFree(darena);
		if (dout) (void)hipFree(dout);
		if (stream) (void)hipStreamDestroy(stream);
	}
};

namespace {

std::string g_sg_create_error;

template <class T> hipError_t upload(T** dev, const std::vector<T>& host, hipStream_t stream)
{
	hipError_t e = hipMalloc((void**)dev, std::max<size_t>(host.size(), 1) * sizeof(T));
	if (e == hipSuccess && !host.empty()) e = hipMemcpyAsync(*dev, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice, stream);
	return e;
}

} // namespace

extern "C" {

int abg_sg_create(int device, abg_sg** out)
{
	if (!out) return ABG_EINVAL;
	*out = nullptr;
	hipStream_t stream = nullptr;
	const int rc = st::open_device(device, "path searcher", g_sg_create_error, &stream, 1);
	if (rc != ABG_OK) return rc;
	abg_sg* s = new abg_sg;
	s->device = device;
	s->stream = stream;
	s->batch = st::env_u64("ABG_SG_BATCH", 1, 1ull << 24, s->batch);
	s->stack_depth = (uint32_t)st::env_u64("ABG_SG_STACK_DEPTH", 1, 1u << 16, s->stack_depth);
	s->max_constraints = (uint32_t)st::env_u64("ABG_SG_MAX_CONSTRAINTS", 1, abg::SG_MAX_CONSTRAINTS, s->max_constraints);
	s->arena_words = st::env_u64("ABG_SG_ARENA_WORDS", 1, 1ull << 30, s->arena_words);
	s->max_lanes = (uint32_t)((st::env_u64("ABG_SG_LANES", 1, 1u << 20, s->max_lanes) + 63) / 64 * 64);
	*out = s;
	return ABG_OK;
}

void abg_sg_destroy(abg_sg* s) { delete s; }
const char* abg_sg_last_error(const abg_sg* s) { return s ? s->error.c_str() : g_sg_create_error.c_str(); }

int abg_sg_tune(abg_sg* s, uint32_t stack_depth, uint32_t max_constraints, uint64_t arena_words, uint32_t lanes)
{
	if (!s) return ABG_EINVAL;
	if (stack_depth > (1u << 16) || max_constraints > abg::SG_MAX_CONSTRAINTS || arena_words > (1ull << 30) || lanes > (1u << 20)) {
		s->error = "abg_sg_tune: at most 65536 frames, 64 constraints, 2^30 arena words and 2^20 lanes";
		return ABG_EINVAL;
	}
	if (stack_depth) s->stack_depth = stack_depth;
	if (max_constraints) s->max_constraints = max_constraints;
	if (arena_words) s->arena_words = arena_words;
	if (lanes) s->max_lanes = (lanes + 63) / 64 * 64;
	return ABG_OK;
}

int abg_sg_set_graph(abg_sg* s, uint64_t nv, const uint64_t* edge_offsets, const uint32_t* lengths, const uint32_t* targets, const int32_t* distances)
{
	if (!s || !edge_offsets || (nv && !lengths)) return ABG_EINVAL;
	if (nv >= (1ull << 31)) { s->error = "at most 2^31 - 1 vertices"; return ABG_EINVAL; }
	if (edge_offsets[0] != 0) { s->error = "edge_offsets[0] must be 0"; return ABG_EINVAL; }
	for (uint64_t u = 0; u < nv; ++u)
		if (edge_offsets[u + 1] < edge_offsets[u]) { s->error = "vertex " + std::to_string(u) + ": edge offsets must ascend"; return ABG_EINVAL; }
	const uint64_t ne = edge_offsets[nv];
	if (ne >= (1ull << 32) - 1) { s->error = "at most 2^32 - 2 edges"; return ABG_EINVAL; }
	if (ne && (!targets || !distances)) return ABG_EINVAL;
	for (uint64_t e = 0; e < ne; ++e)
		if (targets[e] >= nv) { s->error = "edge " + std::to_string(e) + ": no such vertex"; return ABG_EINVAL; }
	(void)hipSetDevice(s->device);
	(void)hipStreamSynchronize(s->stream);
	s->free_graph();
	s->voff.resize(nv + 1);
	for (uint64_t u = 0; u <= nv; ++u) s->voff[u] = (uint32_t)edge_offsets[u];
	s->vlen.assign(lengths, lengths + nv);
	s->etgt.assign(targets, targets + ne);
	s->edist.assign(distances, distances + ne);
	hipError_t e = upload(&s->d_voff, s->voff, s->stream);
	if (e == hipSuccess) e = upload(&s->d_vlen, s->vlen, s->stream);
	if (e == hipSuccess) e = upload(&s->d_etgt, s->etgt, s->stream);
	if (e == hipSuccess) e = upload(&s->d_edist, s->edist, s->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
	if (e != hipSuccess) { s->free_graph(); return st::fail(s->error, e, "uploading the graph"); }
	s->have_graph = true;
	return ABG_OK;
}

int abg_sg_search(abg_sg* s, uint64_t nsearch, const uint32_t* origins, const uint64_t* constraint_offsets, const uint32_t* constraint_vertices,
    const int32_t* constraint_bounds, uint32_t max_cost, uint32_t max_paths, uint32_t* visited, uint8_t* redone, uint64_t* path_index,
    const uint64_t** path_offsets, const uint32_t** path_nodes)
{
	if (!s || !path_index || !path_offsets || !path_nodes) return ABG_EINVAL;
	s->path_off.assign(1, 0);
	s->nodes.clear();
	path_index[0] = 0;
	*path_offsets = s->path_off.data();
	*path_nodes = s->nodes.data();
	if (nsearch == 0) return ABG_OK;
	if (!origins || !constraint_offsets || !visited || !redone) return ABG_EINVAL;
	if (!s->have_graph) { s->error = "no graph has been set"; return ABG_EINVAL; }
	if (nsearch >= (1ull << 32) - 1) { s->error = "at most 2^32 - 2 searches a call"; return ABG_EINVAL; }
	const uint32_t nv = (uint32_t)s->vlen.size();
	if (constraint_offsets[0] != 0) { s->error = "constraint_offsets[0] must be 0"; return ABG_EINVAL; }
	const uint64_t ncall = constraint_offsets[nsearch];
	for (uint64_t i = 0; i < nsearch; ++i) {
		if (origins[i] >= nv) { s->error = "search " + std::to_string(i) + ": no such vertex"; return ABG_EINVAL; }
		if (constraint_offsets[i + 1] < constraint_offsets[i] || constraint_offsets[i + 1] - constraint_offsets[i] > 0x7FFFFFFFull) {
			s->error = "search " + std::to_string(i) + ": constraint offsets must ascend";
			return ABG_EINVAL;
		}
	}
	if (ncall >= (1ull << 32)) { s->error = "at most 2^32 - 1 constraints a call"; return ABG_EINVAL; }
	if (ncall && (!constraint_vertices || !constraint_bounds)) return ABG_EINVAL;
	for (uint64_t c = 0; c < ncall; ++c)
		if (constraint_vertices[c] >= nv) { s->error = "constraint " + std::to_string(c) + ": no such vertex"; return ABG_EINVAL; }
	// the constraints of every search, sorted as ConstrainedSearch.h:134 sorts them
	std::vector<uint32_t> cv(constraint_vertices, constraint_vertices + ncall);
	std::vector<int32_t> cb(constraint_bounds, constraint_bounds + ncall);
	for (uint64_t i = 0; i < nsearch; ++i)
		abg::sg_sort_constraints(cv.data() + constraint_offsets[i], cb.data() + constraint_offsets[i], (uint32_t)(constraint_offsets[i + 1] - constraint_offsets[i]));
	std::vector<uint32_t> status(nsearch, abg::SG_DONE);
	std::vector<uint64_t> device; // the searches the device takes
	for (uint64_t i = 0; i < nsearch; ++i) {
		const uint64_t nc = constraint_offsets[i + 1] - constraint_offsets[i];
		visited[i] = 0;
		redone[i] = 0;
		if (nc == 0) continue; // ConstrainedSearch.h:130-131: nothing is searched
		if (nc > s->max_constraints) status[i] = abg::SG_ECONSTRAINTS;
		else device.push_back(i);
	}
	(void)hipSetDevice(s->device);
	hipError_t e = hipSuccess;
	if (!device.empty()) {
		e = st::grow(&s->din, &s->in_cap, std::max<size_t>(ncall, 1) * 8 + 64);
		if (e == hipSuccess) e = hipMemcpyAsync(s->din, cv.data(), ncall * 4, hipMemcpyHostToDevice, s->stream);
		if (e == hipSuccess) e = hipMemcpyAsync((uint32_t*)s->din + ncall, cb.data(), ncall * 4, hipMemcpyHostToDevice, s->stream);
		if (e != hipSuccess) return st::fail(s->error, e, "copying the constraints to the device");
	}
	const abg::SGGraph dg{ s->d_voff, s->d_vlen, s->d_etgt, s->d_edist, nv };
	// per search the arena records of its paths, in discovery order: (offset into the batch's arena copy, length)
	std::vector<std::vector<uint32_t>> found(nsearch);
	std::vector<abg::SGJob> jobs;
	std::vector<uint32_t> harena, hvis, hstat;
	int rc = ABG_OK;
	// The searches still to launch, from `head` on.  A launch that fills its arena flags every search that then finds a path; those
	// go out again with the searches after them, and when a whole launch is flagged its searches go out fewer at a time.  Only a
	// search that fills the arena on its own is left flagged for the host.
	std::vector<uint64_t> work(device), chunk, again;
	size_t head = 0;
	uint64_t limit = s->batch;
	while (head < work.size() && rc == ABG_OK) {
		const uint64_t nb = std::min<uint64_t>(work.size() - head, limit);
		chunk.assign(work.begin() + head, work.begin() + head + nb);
		jobs.resize(nb);
		for (uint64_t i = 0; i < nb; ++i) {
			const uint64_t q = chunk[i];
			jobs[i] = abg::SGJob{ origins[q], (uint32_t)constraint_offsets[q], (uint32_t)(constraint_offsets[q + 1] - constraint_offsets[q]), 0 };
		}
		const uint32_t lanes = (uint32_t)std::min<uint64_t>((nb + 63) / 64 * 64, s->max_lanes);
		// jobs, then the three counters and the arena cursor, then visited and status
		const size_t jobs_bytes = (nb * sizeof(abg::SGJob) + 63) & ~(size_t)63;
		e = st::grow(&s->dout, &s->out_cap, jobs_bytes + 64 + nb * 8);
		if (e == hipSuccess) e = st::grow(&s->dstack, &s->stack_cap, (size_t)lanes * s->stack_depth * sizeof(uint4));
		if (e == hipSuccess) e = st::grow(&s->darena, &s->arena_cap, (size_t)s->arena_words * 4);
		if (e != hipSuccess) { rc = st::fail(s->error, e, "allocating a batch"); break; }
		char* base = (char*)s->dout;
		unsigned long long* dcounters = (unsigned long long*)(base + jobs_bytes);
		uint32_t* dvis = (uint32_t*)(base + jobs_bytes + 64);
		uint32_t* dstat = dvis + nb;
		e = hipMemcpyAsync(base, jobs.data(), nb * sizeof(abg::SGJob), hipMemcpyHostToDevice, s->stream);
		const unsigned long long zero[8] = { 0, 0, 0, 0, ~0ull, 0, 0, 0 }; // [3] the arena cursor, [4] where its records end
		if (e == hipSuccess) e = hipMemcpyAsync(dcounters, zero, 64, hipMemcpyHostToDevice, s->stream);
		if (e != hipSuccess) { rc = st::fail(s->error, e, "copying a batch to the device"); break; }
		{
			st::Timed t(s->prof, s->stream, "sg_search", s->profiling != 0);
			hipLaunchKernelGGL(sg_search_kernel, dim3(lanes / 64), dim3(64), 0, s->stream, dg, (const abg::SGJob*)base, (const uint32_t*)s->din,
			    (const int32_t*)((uint32_t*)s->din + ncall), (uint32_t)nb, max_cost, max_paths, (uint4*)s->dstack, s->stack_depth, (uint32_t*)s->darena,
			    (uint64_t)s->arena_words, dcounters + 3, dcounters, dvis, dstat, s->profiling == 2 ? 1 : 0);
			e = hipGetLastError();
		}
		if (e != hipSuccess) { rc = st::fail(s->error, e, "launching the search"); break; }
		unsigned long long hc[5] = { 0, 0, 0, 0, 0 };
		hvis.resize(nb); hstat.resize(nb);
		e = hipMemcpyAsync(hc, dcounters, 40, hipMemcpyDeviceToHost, s->stream);
		if (e == hipSuccess) e = hipMemcpyAsync(hvis.data(), dvis, nb * 4, hipMemcpyDeviceToHost, s->stream);
		if (e == hipSuccess) e = hipMemcpyAsync(hstat.data(), dstat, nb * 4, hipMemcpyDeviceToHost, s->stream);
		if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
		if (e != hipSuccess) { rc = st::fail(s->error, e, "the search"); break; }
		s->thin_steps += hc[1];
		s->all_steps += hc[2];
		const uint64_t used = std::min<uint64_t>(std::min<uint64_t>(hc[3], hc[4]), s->arena_words);
		harena.resize(used);
		if (used) {
			e = hipMemcpy(harena.data(), s->darena, used * 4, hipMemcpyDeviceToHost);
			if (e != hipSuccess) { rc = st::fail(s->error, e, "copying the paths back"); break; }
		}
		again.clear();
		for (uint64_t i = 0; i < nb; ++i) {
			const uint64_t q = chunk[i];
			visited[q] = hvis[i];
			status[q] = hstat[i];
			if (hstat[i] == abg::SG_EARENA) again.push_back(q);
		}
		// the records lie end to end; the first one that did not fit ends them
		for (uint64_t off = 0; off + 2 <= used;) {
			const uint32_t which = harena[off], len = harena[off + 1];
			if (which >= nb || len == 0 || off + 2 + len > used) break;
			const uint64_t q = chunk[which];
			if (status[q] == abg::SG_DONE) {
				std::vector<uint32_t>& f = found[q];
				f.push_back(len);
				f.insert(f.end(), harena.begin() + off + 2, harena.begin() + off + 2 + len);
			}
			off += 2 + (uint64_t)len;
		}
		if (again.size() < nb) {
			head += nb - again.size(); // (the flagged ones take the last places of this launch, and go first in the next)
			std::copy(again.begin(), again.end(), work.begin() + head);
			limit = s->batch;
		} else if (nb > 1)
			limit = nb / 2;
		else
			head += 1;
	}
	if (rc != ABG_OK) { (void)hipStreamSynchronize(s->stream); return rc; }
	// the flagged searches again, on the host, and everything in the caller's order
	const abg::SGGraph hg{ s->voff.data(), s->vlen.data(), s->etgt.data(), s->edist.data(), nv };
	std::vector<uint64_t> ends;
	for (uint64_t i = 0; i < nsearch; ++i) {
		if (status[i] != abg::SG_DONE) {
			redone[i] = 1;
			s->redone++;
			ends.clear();
			abg::sg_search_host(hg, origins[i], cv.data() + constraint_offsets[i], cb.data() + constraint_offsets[i],
			    (uint32_t)(constraint_offsets[i + 1] - constraint_offsets[i]), max_cost, max_paths, &visited[i], s->nodes, ends);
			for (uint64_t x : ends) s->path_off.push_back(x);
		} else {
			const std::vector<uint32_t>& f = found[i];
			for (size_t p = 0; p < f.size(); p += 1 + f[p]) {
				s->nodes.insert(s->nodes.end(), f.begin() + p + 1, f.begin() + p + 1 + f[p]);
				s->path_off.push_back(s->nodes.size());
			}
		}
		path_index[i + 1] = s->path_off.size() - 1;
	}
	*path_offsets = s->path_off.data();
	*path_nodes = s->nodes.data();
	return ABG_OK;
}

int abg_sg_profile(abg_sg* s, int on)
{
	if (!s) return ABG_EINVAL;
	s->profiling = on < 0 ? 0 : on > 2 ? 2 : on;
	return ABG_OK;
}

int abg_sg_profile_get(abg_sg* s, const char* name, double* total_ms, uint64_t* launches)
{
	if (!s || !name) return ABG_EINVAL;
	(void)hipSetDevice(s->device);
	if (total_ms) *total_ms = 0;
	// not kernels: wave steps of the profiled calls, those taken with fewer than half the lanes busy, and searches redone on the host
	if (!strcmp(name, "sg_steps")) { if (launches) *launches = s->all_steps; return ABG_OK; }
	if (!strcmp(name, "sg_thin_steps")) { if (launches) *launches = s->thin_steps; return ABG_OK; }
	if (!strcmp(name, "sg_redone")) { if (launches) *launches = s->redone; return ABG_OK; }
	return s->prof.get(name, total_ms, launches);
}

} // extern "C"
