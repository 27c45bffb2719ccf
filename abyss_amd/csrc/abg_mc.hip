// abg_mc.hip -- MergeContigs' sequence merge on the GPU and the abg_mc_* entry points (include/abyss_amd.h).
//
// Two kernels a batch of paths (abg_mc.h says why):
//   mc_junction_kernel  a wave a path.  It walks the junctions in order with the last characters of the sequence so far in an LDS
//                       ring (position p of the sequence at ring[p % MC_RING]), lanes over the overlap window: consensus of the ring's
//                       tail and the head of the next node, written back to the ring and to the side buffer; then the node's remaining
//                       characters, as many as a later window can reach, are appended to the ring.  The first junction with no
//                       consensus flags the path and ends it.
//   mc_splice_kernel    flat over the output bytes of the whole batch, a block a tile, a thread sixteen bytes at a time.  A thread
//                       finds its segment by binary search between the tile's first and last; sixteen bytes inside one segment are
//                       two 8-byte words built from aligned loads (reversed and complemented through a table in LDS for a contig read
//                       backwards) and one 16-byte store; sixteen bytes across a seam go byte by byte.  It counts the ACGT of every
//                       output contig.  Its work is the output bytes, whatever the lengths of paths and contigs.
// The host lays out the segments (mc_layout) before either kernel runs, so nothing comes back between them; a flagged path's bytes
// are written anyway and replaced by mc_merge_path_host's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/abyss_amd.h"
#include "abg_mc.h"
#include "abg_stage.h"

namespace st = abg::stage;

namespace {

// a path as the junction kernel takes it: its nodes and overlaps at first .. first + n of the batch's arrays, its consensus
// characters from `side` on, the longest of its overlaps, and whether the host has taken it already
struct MCPath { uint64_t first, side; uint32_t n, window, skip, pad; };

__global__ __launch_bounds__(64) void mc_junction_kernel(abg::MCStore st, uint32_t k, const MCPath* __restrict__ paths, const int32_t* __restrict__ nodes,
    const uint32_t* __restrict__ ov, uint8_t* __restrict__ side, uint32_t* __restrict__ flags)
{
	__shared__ uint8_t ring[abg::MC_RING];
	const MCPath p = paths[blockIdx.x];
	if (p.skip || p.n < 2) return;
	const uint32_t lane = threadIdx.x;
	const int32_t* nd = nodes + p.first;
	const uint32_t* o = ov + p.first;
	uint64_t end = abg::mc_node_len(st, nd[0], k), soff = p.side;
	{
		const uint64_t cnt = end < p.window ? end : p.window;
		for (uint64_t q = lane; q < cnt; q += 64) {
			const uint64_t pos = end - cnt + q;
			ring[pos & (abg::MC_RING - 1)] = abg::mc_node_char(st, nd[0], k, pos);
		}
	}
	__syncthreads();
	for (uint32_t j = 1; j < p.n; ++j) {
		const uint32_t w = o[j];
		const int32_t node = nd[j];
		const uint64_t len = abg::mc_node_len(st, node, k);
		int bad = 0;
		for (uint32_t q = lane; q < w; q += 64) {
			const uint64_t pos = end - w + q;
			const uint8_t c = abg::mc_consensus_char(ring[pos & (abg::MC_RING - 1)], abg::mc_node_char(st, node, k, q));
			if (c == 0) bad = 1;
			else { ring[pos & (abg::MC_RING - 1)] = c; side[soff + q] = c; }
		}
		if (__syncthreads_or(bad)) { if (lane == 0) flags[blockIdx.x] = 1; return; }
		soff += w;
		const uint64_t rest = len - w, cnt = rest < p.window ? rest : p.window;
		for (uint64_t q = lane; q < cnt; q += 64) {
			const uint64_t at = rest - cnt + q;
			ring[(end + at) & (abg::MC_RING - 1)] = abg::mc_node_char(st, node, k, w + at);
		}
		end += rest;
		__syncthreads();
	}
}

// the sixteen bytes at byte position pos of the 8-byte words w, lowest address in the lowest byte of lo
__device__ __forceinline__ void load16(const uint64_t* __restrict__ w, uint64_t pos, uint64_t& lo, uint64_t& hi)
{
	const uint64_t i = pos >> 3;
	const unsigned s = (unsigned)(pos & 7) * 8;
	const uint64_t a = w[i], b = w[i + 1];
	if (s == 0) { lo = a; hi = b; return; }
	const uint64_t c = w[i + 2];
	lo = (a >> s) | (b << (64 - s));
	hi = (b >> s) | (c << (64 - s));
}

__device__ __forceinline__ uint32_t count_acgt(uint64_t x, uint32_t nbytes)
{
	uint32_t n = 0;
	for (uint32_t i = 0; i < nbytes; ++i) n += abg::mc_acgt((uint8_t)(x >> (8 * i))) ? 1u : 0u;
	return n;
}

// the last segment of [lo, hi] that starts at or before pos (segs[lo].start <= pos)
__device__ __forceinline__ uint64_t find_seg(const abg::MCSeg* __restrict__ segs, uint64_t lo, uint64_t hi, uint64_t pos)
{
	while (lo < hi) {
		const uint64_t mid = lo + (hi - lo + 1) / 2;
		if (segs[mid].start <= pos) lo = mid; else hi = mid - 1;
	}
	return lo;
}

// store: the padded store as words (byte position MC_PAD + offset); sidew: the side buffer as words
__global__ __launch_bounds__(abg::MC_BLOCK) void mc_splice_kernel(const uint64_t* __restrict__ store, const uint64_t* __restrict__ sidew,
    const abg::MCSeg* __restrict__ segs, uint64_t nsegs, uint64_t total, uint64_t tile, uint8_t* __restrict__ out, unsigned long long* __restrict__ acgt)
{
	__shared__ uint8_t comp[256];
	__shared__ uint64_t range[2];
	const uint64_t t0 = (uint64_t)blockIdx.x * tile, t1 = t0 + tile < total ? t0 + tile : total;
	comp[threadIdx.x] = abg::ov_complement((uint8_t)threadIdx.x);
	if (threadIdx.x < 2) range[threadIdx.x] = find_seg(segs, 0, nsegs - 1, threadIdx.x == 0 ? t0 : t1 - 1);
	__syncthreads();
	const uint8_t* storeb = (const uint8_t*)store;
	const uint8_t* sideb = (const uint8_t*)sidew;
	unsigned long long mine = 0;
	uint32_t mine_path = 0;
	auto credit = [&](uint32_t path, uint32_t n) {
		if (n == 0) return;
		if (path != mine_path && mine) { atomicAdd(&acgt[mine_path], mine); mine = 0; }
		mine_path = path;
		mine += n;
	};
	for (uint64_t c = t0 + (uint64_t)threadIdx.x * 16; c < t1; c += (uint64_t)abg::MC_BLOCK * 16) {
		const uint32_t n = (uint32_t)(t1 - c < 16 ? t1 - c : 16);
		uint64_t s = find_seg(segs, range[0], range[1], c);
		abg::MCSeg g = segs[s];
		uint64_t next = s + 1 < nsegs ? segs[s + 1].start : total;
		uint64_t lo = 0, hi = 0;
		if (next >= c + n) { // the whole of it in one segment
			const uint64_t d = c - g.start;
			if (g.kind == abg::MC_SEG_FORWARD) load16(store, abg::MC_PAD + g.src + d, lo, hi);
			else if (g.kind == abg::MC_SEG_CONSENSUS) load16(sidew, g.src + d, lo, hi);
			else if (g.kind == abg::MC_SEG_REVERSE) {
				uint64_t a, b;
				load16(store, abg::MC_PAD + g.src - d - 15, a, b);
				for (int i = 0; i < 8; ++i) {
					lo |= (uint64_t)comp[(b >> (56 - 8 * i)) & 0xff] << (8 * i);
					hi |= (uint64_t)comp[(a >> (56 - 8 * i)) & 0xff] << (8 * i);
				}
			} else lo = hi = 0x0101010101010101ull * (g.src & 0xff);
			credit(g.path, count_acgt(lo, n < 8 ? n : 8) + (n > 8 ? count_acgt(hi, n - 8) : 0));
		} else {
			for (uint32_t i = 0; i < n; ++i) {
				const uint64_t pos = c + i;
				while (next <= pos) { g = segs[++s]; next = s + 1 < nsegs ? segs[s + 1].start : total; }
				const uint64_t d = pos - g.start;
				uint8_t ch;
				if (g.kind == abg::MC_SEG_FORWARD) ch = storeb[abg::MC_PAD + g.src + d];
				else if (g.kind == abg::MC_SEG_CONSENSUS) ch = sideb[g.src + d];
				else if (g.kind == abg::MC_SEG_REVERSE) ch = comp[storeb[abg::MC_PAD + g.src - d]];
				else ch = (uint8_t)g.src;
				if (i < 8) lo |= (uint64_t)ch << (8 * i); else hi |= (uint64_t)ch << (8 * (i - 8));
				credit(g.path, abg::mc_acgt(ch) ? 1u : 0u);
			}
		}
		*(ulonglong2*)(out + c) = make_ulonglong2(lo, hi);
	}
	if (mine) atomicAdd(&acgt[mine_path], mine);
}

} // namespace

struct abg_mc {
	int device = 0;
	hipStream_t stream = nullptr;
	// the store on both sides: MC_PAD zero bytes, the contigs, MC_PAD zero bytes
	std::vector<uint8_t> store;
	std::vector<uint64_t> off;
	std::vector<uint8_t> reversible; // per contig: every byte has a complement
	uint8_t* d_store = nullptr; uint64_t* d_off = nullptr;
	bool have_contigs = false;
	uint64_t tile = 16384, batch = 1ull << 20;
	void* din = nullptr; size_t in_cap = 0;    // paths, nodes, overlaps, segments
	void* dside = nullptr; size_t side_cap = 0;
	void* dout = nullptr; size_t out_cap = 0;  // flags, counts, then the output bytes
	// the answer of the last call
	std::vector<uint8_t> seqs;
	std::string logs;
	int profiling = 0;
	st::Profile prof;
	uint64_t redone = 0, bytes = 0;
	std::string error;
	void free_contigs()
	{
		if (d_store) (void)hipFree(d_store);
		if (d_off) (void)hipFree(d_off);
		d_store = nullptr;
		d_off = nullptr;
		have_contigs = false;
	}
	~abg_mc()
	{
		(void)hipSetDevice(device);
		if (stream) (void)hipStreamSynchronize(stream);
		prof.drop();
		free_contigs();
		if (din) (void)hipFree(din);
		if (dside) (void)hipFree(dside);
		if (dout) (void)hipFree(dout);
		if (stream) (void)hipStreamDestroy(stream);
	}
};

namespace {

std::string g_mc_create_error;

} // namespace

extern "C" {

int abg_mc_create(int device, abg_mc** out)
{
	if (!out) return ABG_EINVAL;
	*out = nullptr;
	hipStream_t stream = nullptr;
	const int rc = st::open_device(device, "path merger", g_mc_create_error, &stream, 1);
	if (rc != ABG_OK) return rc;
	abg_mc* s = new abg_mc;
	s->device = device;
	s->stream = stream;
	s->tile = st::env_u64("ABG_MC_TILE", 16, 1ull << 24, s->tile) / 16 * 16;
	s->batch = st::env_u64("ABG_MC_BATCH", 1, 1ull << 24, s->batch);
	*out = s;
	return ABG_OK;
}

void abg_mc_destroy(abg_mc* s) { delete s; }
const char* abg_mc_last_error(const abg_mc* s) { return s ? s->error.c_str() : g_mc_create_error.c_str(); }

int abg_mc_tune(abg_mc* s, uint64_t tile, uint64_t batch)
{
	if (!s) return ABG_EINVAL;
	if (tile > (1ull << 24) || batch > (1ull << 24) || (tile && (tile < 16 || tile % 16))) {
		s->error = "abg_mc_tune: a tile is a multiple of 16 bytes up to 2^24, a batch at most 2^24 paths";
		return ABG_EINVAL;
	}
	if (tile) s->tile = tile;
	if (batch) s->batch = batch;
	return ABG_OK;
}

int abg_mc_set_contigs(abg_mc* s, const uint8_t* bytes, const uint64_t* offsets, uint64_t n)
{
	if (!s || !offsets || (n && offsets[n] && !bytes)) return ABG_EINVAL;
	if (n >= (1ull << 30)) { s->error = "at most 2^30 - 1 contigs"; return ABG_EINVAL; }
	if (offsets[0] != 0) { s->error = "offsets[0] must be 0"; return ABG_EINVAL; }
	for (uint64_t i = 0; i < n; ++i)
		if (offsets[i + 1] < offsets[i]) { s->error = "contig " + std::to_string(i) + ": offsets must ascend"; return ABG_EINVAL; }
	const uint64_t total = offsets[n];
	(void)hipSetDevice(s->device);
	(void)hipStreamSynchronize(s->stream);
	s->free_contigs();
	s->store.assign(st::up(total + 2 * abg::MC_PAD, 8), 0);
	if (total) memcpy(s->store.data() + abg::MC_PAD, bytes, total);
	s->off.assign(offsets, offsets + n + 1);
	s->reversible.assign(n, 1);
	uint8_t valid[256];
	for (int c = 0; c < 256; ++c) valid[c] = abg::ov_complement((uint8_t)c) != 0;
	for (uint64_t i = 0; i < n; ++i)
		for (uint64_t p = offsets[i]; p < offsets[i + 1]; ++p)
			if (!valid[bytes[p]]) { s->reversible[i] = 0; break; }
	hipError_t e = hipMalloc((void**)&s->d_store, s->store.size());
	if (e == hipSuccess) e = hipMalloc((void**)&s->d_off, (n + 1) * 8);
	if (e == hipSuccess) e = hipMemcpyAsync(s->d_store, s->store.data(), s->store.size(), hipMemcpyHostToDevice, s->stream);
	if (e == hipSuccess) e = hipMemcpyAsync(s->d_off, s->off.data(), (n + 1) * 8, hipMemcpyHostToDevice, s->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
	if (e != hipSuccess) { s->free_contigs(); return st::fail(s->error, e, "uploading the contigs"); }
	s->have_contigs = true;
	return ABG_OK;
}

int abg_mc_merge(abg_mc* s, uint32_t k, uint64_t npaths, const uint64_t* node_offsets, const int32_t* nodes, const uint32_t* overlaps, int verbose,
    uint8_t* redone, uint64_t* seq_offsets, const uint8_t** seqs, uint64_t* acgt, uint64_t* log_offsets, const char** logs)
{
	if (!s || !seq_offsets || !seqs || !log_offsets || !logs) return ABG_EINVAL;
	s->seqs.clear();
	s->logs.clear();
	seq_offsets[0] = 0;
	log_offsets[0] = 0;
	*seqs = s->seqs.data();
	*logs = s->logs.c_str();
	if (npaths == 0) return ABG_OK;
	if (!node_offsets || !redone || !acgt) return ABG_EINVAL;
	if (!s->have_contigs) { s->error = "no contigs have been set"; return ABG_EINVAL; }
	if (k == 0) { s->error = "k must be positive"; return ABG_EINVAL; }
	if (node_offsets[0] != 0) { s->error = "node_offsets[0] must be 0"; return ABG_EINVAL; }
	const uint64_t ncontigs = s->off.size() - 1;
	for (uint64_t i = 0; i < npaths; ++i) {
		if (node_offsets[i + 1] < node_offsets[i] || node_offsets[i + 1] - node_offsets[i] >= (1ull << 32)) {
			s->error = "path " + std::to_string(i) + ": node offsets must ascend";
			return ABG_EINVAL;
		}
		for (uint64_t j = node_offsets[i]; j < node_offsets[i + 1]; ++j) {
			const int32_t u = nodes[j];
			if (u >= 0 && ((uint64_t)u >> 1) >= ncontigs) { s->error = "path " + std::to_string(i) + ": no such contig"; return ABG_EINVAL; }
			if (u >= 0 && (u & 1) && !s->reversible[(uint32_t)u >> 1]) {
				s->error = "path " + std::to_string(i) + ": contig " + std::to_string((uint32_t)u >> 1) + " holds a character that has no complement";
				return ABG_EINVAL;
			}
			if (u < 0 && (uint64_t)(-(int64_t)u) + k > 0x7fffffffull) { s->error = "path " + std::to_string(i) + ": the gap is too long"; return ABG_EINVAL; }
			if (j > node_offsets[i] && overlaps[j] == 0) { s->error = "path " + std::to_string(i) + ": an overlap must be positive"; return ABG_EINVAL; }
		}
	}
	(void)hipSetDevice(s->device);
	const abg::MCStore hs{ s->store.data() + abg::MC_PAD, s->off.data(), ncontigs };
	const abg::MCStore ds{ s->d_store + abg::MC_PAD, s->d_off, ncontigs };
	std::vector<MCPath> paths;
	std::vector<abg::MCSeg> segs;
	std::vector<uint64_t> lengths;
	std::vector<uint32_t> flags;
	std::vector<unsigned long long> counts;
	std::string seq, log;
	for (uint64_t b0 = 0; b0 < npaths; b0 += s->batch) {
		const uint64_t nb = std::min<uint64_t>(s->batch, npaths - b0), n0 = node_offsets[b0], nn = node_offsets[b0 + nb] - n0;
		paths.assign(nb, MCPath{ 0, 0, 0, 0, 0, 0 });
		lengths.assign(nb, 0);
		segs.clear();
		uint64_t total = 0, side = 0;
		for (uint64_t i = 0; i < nb; ++i) {
			const uint64_t first = node_offsets[b0 + i] - n0, n = node_offsets[b0 + i + 1] - node_offsets[b0 + i];
			uint32_t window = 0;
			for (uint64_t j = 1; j < n; ++j) window = std::max(window, overlaps[n0 + first + j]);
			MCPath& p = paths[i];
			p = MCPath{ first, side, (uint32_t)n, window, 0, 0 };
			const size_t mark = segs.size();
			// a window the ring cannot hold, or an overlap the reference asserts on: the host's from the start
			if (window > abg::MC_RING || !abg::mc_layout(hs, k, nodes + n0 + first, overlaps + n0 + first, n, (uint32_t)i, total, side, segs, &lengths[i])) {
				segs.resize(mark);
				lengths[i] = 0;
				p.skip = 1;
				continue;
			}
			for (uint64_t j = 1; j < n; ++j) side += overlaps[n0 + first + j];
			total += lengths[i];
		}
		flags.assign(nb, 0);
		counts.assign(nb, 0);
		const size_t base = s->seqs.size();
		if (total > 0) {
			// the input block: paths, segments, nodes, overlaps; the output block: flags, counts, bytes
			const size_t paths_at = 0, segs_at = st::up(nb * sizeof(MCPath), 64), nodes_at = segs_at + st::up(segs.size() * sizeof(abg::MCSeg), 64),
			             ov_at = nodes_at + st::up(nn * 4, 64), in_bytes = ov_at + st::up(nn * 4, 64);
			const size_t flags_at = 0, counts_at = st::up(nb * 4, 64), out_at = counts_at + st::up(nb * 8, 64), out_bytes = out_at + st::up(total, 16);
			hipError_t e = st::grow(&s->din, &s->in_cap, in_bytes);
			if (e == hipSuccess) e = st::grow(&s->dside, &s->side_cap, st::up(side, 8) + 64);
			if (e == hipSuccess) e = st::grow(&s->dout, &s->out_cap, out_bytes);
			if (e != hipSuccess) return st::fail(s->error, e, "allocating a batch");
			char* in = (char*)s->din;
			char* out = (char*)s->dout;
			e = hipMemcpyAsync(in + paths_at, paths.data(), nb * sizeof(MCPath), hipMemcpyHostToDevice, s->stream);
			if (e == hipSuccess) e = hipMemcpyAsync(in + segs_at, segs.data(), segs.size() * sizeof(abg::MCSeg), hipMemcpyHostToDevice, s->stream);
			if (e == hipSuccess && nn) e = hipMemcpyAsync(in + nodes_at, nodes + n0, nn * 4, hipMemcpyHostToDevice, s->stream);
			if (e == hipSuccess && nn) e = hipMemcpyAsync(in + ov_at, overlaps + n0, nn * 4, hipMemcpyHostToDevice, s->stream);
			if (e == hipSuccess) e = hipMemsetAsync(out, 0, out_at, s->stream);
			if (e != hipSuccess) return st::fail(s->error, e, "copying a batch to the device");
			if (side > 0) {
				st::Timed t(s->prof, s->stream, "mc_junction", s->profiling != 0);
				hipLaunchKernelGGL(mc_junction_kernel, dim3((unsigned)nb), dim3(64), 0, s->stream, ds, k, (const MCPath*)(in + paths_at), (const int32_t*)(in + nodes_at),
				    (const uint32_t*)(in + ov_at), (uint8_t*)s->dside, (uint32_t*)(out + flags_at));
				e = hipGetLastError();
			}
			if (e != hipSuccess) return st::fail(s->error, e, "launching the junction pass");
			{
				st::Timed t(s->prof, s->stream, "mc_splice", s->profiling != 0);
				const uint64_t tiles = (total + s->tile - 1) / s->tile;
				hipLaunchKernelGGL(mc_splice_kernel, dim3((unsigned)tiles), dim3(abg::MC_BLOCK), 0, s->stream, (const uint64_t*)s->d_store, (const uint64_t*)s->dside,
				    (const abg::MCSeg*)(in + segs_at), (uint64_t)segs.size(), total, s->tile, (uint8_t*)(out + out_at), (unsigned long long*)(out + counts_at));
				e = hipGetLastError();
			}
			if (e != hipSuccess) return st::fail(s->error, e, "launching the splice pass");
			s->seqs.resize(base + total);
			e = hipMemcpyAsync(flags.data(), out + flags_at, nb * 4, hipMemcpyDeviceToHost, s->stream);
			if (e == hipSuccess) e = hipMemcpyAsync(counts.data(), out + counts_at, nb * 8, hipMemcpyDeviceToHost, s->stream);
			if (e == hipSuccess) e = hipMemcpyAsync(s->seqs.data() + base, out + out_at, total, hipMemcpyDeviceToHost, s->stream);
			if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
			if (e != hipSuccess) return st::fail(s->error, e, "the merge");
			s->bytes += total;
		}
		// the flagged paths again, on the host; when there is one, the batch's bytes are put together path by path
		bool any = false;
		for (uint64_t i = 0; i < nb; ++i) any = any || flags[i] || paths[i].skip;
		std::vector<uint8_t> device;
		if (any) { device.assign(s->seqs.begin() + base, s->seqs.end()); s->seqs.resize(base); }
		uint64_t from = 0;
		for (uint64_t i = 0; i < nb; ++i) {
			const uint64_t q = b0 + i;
			redone[q] = flags[i] || paths[i].skip;
			acgt[q] = counts[i];
			if (redone[q]) {
				s->redone++;
				log.clear();
				if (!abg::mc_merge_path_host(hs, k, nodes + n0 + paths[i].first, overlaps + n0 + paths[i].first, paths[i].n, verbose, seq, log, s->error)) {
					s->error = "path " + std::to_string(q) + ": " + s->error;
					return ABG_EINVAL;
				}
				s->seqs.insert(s->seqs.end(), seq.begin(), seq.end());
				s->logs += log;
				acgt[q] = (uint64_t)std::count_if(seq.begin(), seq.end(), [](char c) { return abg::mc_acgt((uint8_t)c); });
			} else if (any)
				s->seqs.insert(s->seqs.end(), device.begin() + from, device.begin() + from + lengths[i]);
			from += lengths[i];
			seq_offsets[q + 1] = any ? s->seqs.size() : base + from;
			log_offsets[q + 1] = s->logs.size();
		}
	}
	*seqs = s->seqs.data();
	*logs = s->logs.c_str();
	return ABG_OK;
}

int abg_mc_profile(abg_mc* s, int on)
{
	if (!s) return ABG_EINVAL;
	s->profiling = on > 0 ? 1 : 0;
	return ABG_OK;
}

int abg_mc_profile_get(abg_mc* s, const char* name, double* total_ms, uint64_t* launches)
{
	if (!s || !name) return ABG_EINVAL;
	(void)hipSetDevice(s->device);
	if (total_ms) *total_ms = 0;
	// not kernels: the paths merged again on the host, and the bytes the splice pass wrote
	if (!strcmp(name, "mc_redone")) { if (launches) *launches = s->redone; return ABG_OK; }
	if (!strcmp(name, "mc_bytes")) { if (launches) *launches = s->bytes; return ABG_OK; }
	return s->prof.get(name, total_ms, launches);
}

} // extern "C"
