// abg_pb.hip -- PopBubbles' global alignment on the GPU and the abg_pb_* entry points (include/abyss_amd.h).
//
// Two kernels a launch (abg_pb.h has the cell, the flags and the traceback they share with the host):
//   pb_lane_kernel  a lane a pair, for pairs whose longer side is at most small_limit (a SNP bubble is 1 x 1, and they come in
//                   tens of thousands).  The lane's two rows of f and g live in LDS, column-major over the lanes so that the 64
//                   lanes of a wave touch 64 banks.  It writes its flags and walks them back itself.
//   pb_wave_kernel  a wave a pair.  Rows go in stripes of 64, lane l holding row i0 + l + 1, and the wave sweeps anti-diagonals: at
//                   step t lane l is at column t - l + 1.  What a cell needs from the row above (f, g) and the character of its
//                   column come from lane l - 1 by a cross-lane move, its left and diagonal neighbours are the lane's own registers.
//                   Lane 0's row above is the previous stripe's last row: lane 63 hands its (f, g) to the lane of the column's
//                   index mod 64, and every 64 columns the wave stores them as one line of a row buffer in HBM; the next stripe
//                   loads them a line at a time and lane 0 takes its column by a uniform cross-lane read.  The writes trail the
//                   reads of the same buffer by 63 columns or more, so one buffer serves.  A lane packs four cells' flags into a
//                   word before it stores them.  Lane 0 walks the flags back when the last stripe is done.
// The host fills a launch with pairs in order until their flags would overflow the arena (ABG_PB_ARENA_BYTES) or `batch` pairs are
// in, and launches again for the rest; a pair whose flags alone exceed the arena is aligned by pb_align_host.  In a chain
// (abg_pb_align_chain) a round's consensuses stay on the device and are the next round's first sequences; only the sizes and the
// finished consensuses come back.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/abyss_amd.h"
#include "abg_pb.h"
#include "abg_stage.h"

namespace st = abg::stage;

namespace {

using abg::PBPair;

__global__ __launch_bounds__(64) void pb_lane_kernel(const PBPair* __restrict__ pairs, const uint32_t* __restrict__ which, uint32_t n, const uint8_t* __restrict__ in,
    const uint8_t* __restrict__ prev, uint8_t* __restrict__ arena, uint8_t* __restrict__ cons, uint32_t* __restrict__ matches, uint32_t* __restrict__ sizes)
{
	__shared__ int rowf[abg::PB_SMALL_MAX + 1][64], rowg[abg::PB_SMALL_MAX + 1][64];
	const uint32_t lane = threadIdx.x, q = blockIdx.x * 64 + lane;
	if (q >= n) return;
	const uint32_t id = which[q];
	const PBPair p = pairs[id];
	const uint8_t* a = (p.a_src ? prev : in) + p.a_off;
	const uint8_t* b = in + p.b_off;
	const uint32_t la = p.la, lb = p.lb;
	const uint64_t stride = abg::pb_stride(lb);
	uint8_t* fl = arena + p.flag_off;
	for (uint32_t i = 1; i <= la && lb <= abg::PB_SMALL_MAX; i++) { // (a longer b comes here only with an empty a: the rows stay in bounds)
		const uint8_t ca = a[i - 1];
		int f_diag = abg::pb_edge(i - 1), f_left = abg::pb_edge(i), h_left = abg::PB_NEG;
		for (uint32_t j = 1; j <= lb; j++) {
			const int up_f = i == 1 ? abg::pb_edge(j) : rowf[j][lane], up_g = i == 1 ? abg::PB_NEG : rowg[j][lane];
			uint8_t c;
			int f, g, h;
			fl[(uint64_t)(i - 1) * stride + (j - 1)] = (uint8_t)abg::pb_cell(f_diag, up_f, up_g, f_left, h_left, abg::pb_score(ca, b[j - 1], c), f, g, h);
			rowf[j][lane] = f;
			rowg[j][lane] = g;
			f_diag = up_f;
			f_left = f;
			h_left = h;
		}
	}
	uint32_t m, sz;
	abg::pb_traceback(fl, stride, a, la, b, lb, cons ? cons + p.cons_off + la + lb : nullptr, m, sz);
	matches[id] = m;
	sizes[id] = sz;
}

__global__ __launch_bounds__(64) void pb_wave_kernel(const PBPair* __restrict__ pairs, const uint32_t* __restrict__ which, const uint8_t* __restrict__ in,
    const uint8_t* __restrict__ prev, uint8_t* __restrict__ arena, int2* __restrict__ rows, uint8_t* __restrict__ cons, uint32_t* __restrict__ matches,
    uint32_t* __restrict__ sizes)
{
	const uint32_t id = which[blockIdx.x];
	const PBPair p = pairs[id];
	const uint8_t* a = (p.a_src ? prev : in) + p.a_off;
	const uint8_t* b = in + p.b_off;
	const uint32_t la = p.la, lb = p.lb, lane = threadIdx.x;
	const uint64_t stride = abg::pb_stride(lb);
	uint8_t* fl = arena + p.flag_off;
	int2* row = rows + p.row_off; // row[j - 1]: (f, g) of column j in the last row of the stripe before
	for (uint32_t i0 = 0; i0 < la; i0 += 64) {
		const uint32_t i = i0 + lane + 1, nlive = la - i0 < 64 ? la - i0 : 64;
		const bool live = i <= la, last = i0 + 64 >= la;
		const uint32_t code_a = live ? abg::pb_code(a[i - 1]) : 0;
		uint8_t* myfl = fl + (uint64_t)(live ? i - 1 : 0) * stride;
		int f_diag = abg::pb_edge(i - 1), f_left = abg::pb_edge(i), h_left = abg::PB_NEG, f_mine = 0, g_mine = 0;
		int2 line = make_int2(0, 0), out = make_int2(0, 0);
		uint32_t code_line = 0, code_b = 0, pack = 0;
		const uint32_t steps = lb + nlive - 1;
		for (uint32_t t = 0; t < steps; t++) {
			if ((t & 63) == 0) { // the next 64 columns: their characters, and the row above them
				const uint32_t c = t + lane;
				code_line = c < lb ? abg::pb_code(b[c]) : 0;
				if (i0 > 0 && c < lb) line = row[c];
			}
			int up_f = __shfl_up(f_mine, 1), up_g = __shfl_up(g_mine, 1);
			const uint32_t code_up = __shfl_up(code_b, 1);
			const int line_f = __shfl(line.x, (int)(t & 63)), line_g = __shfl(line.y, (int)(t & 63));
			const uint32_t code_new = __shfl(code_line, (int)(t & 63));
			if (lane == 0) {
				up_f = i0 == 0 ? abg::pb_edge(t + 1) : line_f;
				up_g = i0 == 0 ? abg::PB_NEG : line_g;
				code_b = code_new;
			} else
				code_b = code_up;
			const int j = (int)t - (int)lane + 1;
			if (live && j >= 1 && j <= (int)lb) {
				int f, g, h;
				const uint32_t bits = abg::pb_cell(f_diag, up_f, up_g, f_left, h_left, abg::pb_code_match(code_a, code_b) ? abg::PB_MATCH : abg::PB_MISMATCH, f, g, h);
				f_diag = up_f;
				f_left = f_mine = f;
				g_mine = g;
				h_left = h;
				pack |= bits << (8 * ((j - 1) & 3));
				if ((j & 3) == 0 || j == (int)lb) {
					*(uint32_t*)(myfl + ((uint32_t)(j - 1) & ~3u)) = pack;
					pack = 0;
				}
			}
			if (!last && t >= 63) { // lane 63 has just done column t - 62
				const uint32_t c = t - 63;
				const int of = __shfl(f_mine, 63), og = __shfl(g_mine, 63);
				if (lane == (c & 63)) out = make_int2(of, og);
				if ((c & 63) == 63 || c == lb - 1) {
					const uint32_t at = (c & ~63u) + lane;
					if (at <= c) row[at] = out;
				}
			}
		}
		__syncthreads(); // the row buffer for the next stripe, the flags for the walk
	}
	if (lane == 0) {
		uint32_t m, sz;
		abg::pb_traceback(fl, stride, a, la, b, lb, cons ? cons + p.cons_off + la + lb : nullptr, m, sz);
		matches[id] = m;
		sizes[id] = sz;
	}
}

} // namespace

struct abg_pb {
	int device = 0;
	hipStream_t stream = nullptr;
	uint64_t arena_bytes = 4ull << 30, small_limit = 16, batch = 1ull << 20;
	void* d_in = nullptr; size_t in_cap = 0;        // the input bytes
	void* d_cons[2] = { nullptr, nullptr }; size_t cons_cap[2] = { 0, 0 };
	void* d_meta = nullptr; size_t meta_cap = 0;    // pairs, the two lists, matches, sizes
	void* d_arena = nullptr; size_t arena_cap = 0;
	void* d_rows = nullptr; size_t rows_cap = 0;
	std::vector<uint8_t> cons;                      // the answer of the last call
	st::Profile prof;
	uint64_t redone = 0, cells = 0, launches = 0;
	std::string error;
	~abg_pb()
	{
		(void)hipSetDevice(device);
		if (stream) (void)hipStreamSynchronize(stream);
		prof.drop();
		for (void* p : { d_in, d_cons[0], d_cons[1], d_meta, d_arena, d_rows })
			if (p) (void)hipFree(p);
		if (stream) (void)hipStreamDestroy(stream);
	}
};

namespace {

std::string g_pb_create_error;

constexpr uint64_t PB_MAX_ARENA = 1ull << 40;

// Aligns pairs[0 .. n): a from h_in / d_in (a_src 0) or from d_prev (a_src 1), b from d_in; consensuses to d_out where it is not
// null (each ending at cons_off + la + lb).  flag_off and row_off are filled in here.  matches, sizes, redone: n entries.
int pb_run(abg_pb* s, std::vector<PBPair>& pairs, const uint8_t* h_in, const uint8_t* d_prev, uint8_t* d_out, uint32_t* matches, uint32_t* sizes, uint8_t* redone)
{
	const uint64_t n = pairs.size();
	std::vector<uint32_t> small, large;
	std::vector<uint8_t> ha;
	std::string hc;
	uint64_t q = 0;
	while (q < n) {
		// a launch: pairs from q on while their flags fit
		uint64_t cells = 0, rows = 0, end = q;
		small.clear();
		large.clear();
		for (; end < n && end - q < s->batch; ++end) {
			PBPair& p = pairs[end];
			const uint64_t c = abg::pb_cells(p.la, p.lb);
			if (cells + c > s->arena_bytes) break;
			p.flag_off = cells;
			cells += c;
			const bool lane = p.la == 0 || p.lb == 0 || std::max(p.la, p.lb) <= s->small_limit;
			if (lane) small.push_back((uint32_t)(end - q));
			else { p.row_off = rows; rows += st::up(p.lb, 64); large.push_back((uint32_t)(end - q)); }
		}
		if (end == q) { // the pair at q fits no arena: the host's, by the same header
			PBPair& p = pairs[q];
			const uint8_t* a = h_in + p.a_off;
			if (p.a_src) {
				ha.resize(p.la);
				const hipError_t e = p.la ? hipMemcpy(ha.data(), d_prev + p.a_off, p.la, hipMemcpyDeviceToHost) : hipSuccess;
				if (e != hipSuccess) return st::fail(s->error, e, "fetching a consensus");
				a = ha.data();
			}
			abg::pb_align_host(a, p.la, h_in + p.b_off, p.lb, matches[q], sizes[q], d_out ? &hc : nullptr);
			if (d_out && !hc.empty()) {
				const hipError_t e = hipMemcpy(d_out + p.cons_off + p.la + p.lb - hc.size(), hc.data(), hc.size(), hipMemcpyHostToDevice);
				if (e != hipSuccess) return st::fail(s->error, e, "storing a consensus");
			}
			redone[q] = 1;
			s->redone++;
			++q;
			continue;
		}
		const uint64_t nb = end - q;
		const size_t pairs_at = 0, small_at = st::up(nb * sizeof(PBPair), 64), large_at = small_at + st::up(small.size() * 4, 64), m_at = large_at + st::up(large.size() * 4, 64),
		             s_at = m_at + st::up(nb * 4, 64), meta_bytes = s_at + st::up(nb * 4, 64);
		hipError_t e = st::grow(&s->d_meta, &s->meta_cap, meta_bytes);
		if (e == hipSuccess) e = st::grow(&s->d_arena, &s->arena_cap, std::max<uint64_t>(cells, 64));
		if (e == hipSuccess) e = st::grow(&s->d_rows, &s->rows_cap, std::max<uint64_t>(rows * sizeof(int2), 64));
		if (e != hipSuccess) return st::fail(s->error, e, "allocating a launch");
		char* meta = (char*)s->d_meta;
		e = hipMemcpyAsync(meta + pairs_at, &pairs[q], nb * sizeof(PBPair), hipMemcpyHostToDevice, s->stream);
		if (e == hipSuccess && !small.empty()) e = hipMemcpyAsync(meta + small_at, small.data(), small.size() * 4, hipMemcpyHostToDevice, s->stream);
		if (e == hipSuccess && !large.empty()) e = hipMemcpyAsync(meta + large_at, large.data(), large.size() * 4, hipMemcpyHostToDevice, s->stream);
		if (e != hipSuccess) return st::fail(s->error, e, "copying a launch to the device");
		if (!small.empty()) {
			st::Timed t(s->prof, s->stream, "pb_lane");
			hipLaunchKernelGGL(pb_lane_kernel, dim3((unsigned)((small.size() + 63) / 64)), dim3(64), 0, s->stream, (const PBPair*)(meta + pairs_at),
			    (const uint32_t*)(meta + small_at), (uint32_t)small.size(), (const uint8_t*)s->d_in, d_prev, (uint8_t*)s->d_arena, d_out, (uint32_t*)(meta + m_at),
			    (uint32_t*)(meta + s_at));
			e = hipGetLastError();
		}
		if (e == hipSuccess && !large.empty()) {
			st::Timed t(s->prof, s->stream, "pb_wave");
			hipLaunchKernelGGL(pb_wave_kernel, dim3((unsigned)large.size()), dim3(64), 0, s->stream, (const PBPair*)(meta + pairs_at), (const uint32_t*)(meta + large_at),
			    (const uint8_t*)s->d_in, d_prev, (uint8_t*)s->d_arena, (int2*)s->d_rows, d_out, (uint32_t*)(meta + m_at), (uint32_t*)(meta + s_at));
			e = hipGetLastError();
		}
		if (e != hipSuccess) return st::fail(s->error, e, "launching the alignment");
		e = hipMemcpyAsync(matches + q, meta + m_at, nb * 4, hipMemcpyDeviceToHost, s->stream);
		if (e == hipSuccess) e = hipMemcpyAsync(sizes + q, meta + s_at, nb * 4, hipMemcpyDeviceToHost, s->stream);
		if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
		if (e != hipSuccess) return st::fail(s->error, e, "the alignment");
		for (uint64_t i = q; i < end; ++i) { redone[i] = 0; s->cells += (uint64_t)pairs[i].la * pairs[i].lb; }
		s->launches++;
		s->prof.drain_if(64);
		q = end;
	}
	return ABG_OK;
}

// every byte a code ambiguityToBitmask takes (a digit is colour space, which PopBubbles' drop-in refuses before it gets here)
bool pb_valid(abg_pb* s, const uint8_t* bytes, uint64_t n, const char* what)
{
	uint8_t ok[256];
	for (int c = 0; c < 256; ++c) ok[c] = abg::pb_code((uint8_t)c) != 0;
	for (uint64_t i = 0; i < n; ++i)
		if (!ok[bytes[i]]) { s->error = std::string(what) + ": byte " + std::to_string(i) + " is no nucleotide or IUPAC code"; return false; }
	return true;
}

bool pb_offsets(abg_pb* s, const uint64_t* off, uint64_t n, const char* what)
{
	if (off[0] != 0) { s->error = std::string(what) + "[0] must be 0"; return false; }
	for (uint64_t i = 0; i < n; ++i)
		if (off[i + 1] < off[i] || off[i + 1] - off[i] > 0x3fffffffull) { s->error = std::string(what) + " must ascend, a sequence at most 2^30 - 1 bytes"; return false; }
	return true;
}

} // namespace

extern "C" {

int abg_pb_create(int device, abg_pb** out)
{
	if (!out) return ABG_EINVAL;
	*out = nullptr;
	hipStream_t stream = nullptr;
	const int rc = st::open_device(device, "bubble aligner", g_pb_create_error, &stream, 1);
	if (rc != ABG_OK) return rc;
	abg_pb* s = new abg_pb;
	s->device = device;
	s->stream = stream;
	s->arena_bytes = st::env_u64("ABG_PB_ARENA_BYTES", 4, PB_MAX_ARENA, s->arena_bytes);
	*out = s;
	return ABG_OK;
}

void abg_pb_destroy(abg_pb* s) { delete s; }
const char* abg_pb_last_error(const abg_pb* s) { return s ? s->error.c_str() : g_pb_create_error.c_str(); }

int abg_pb_tune(abg_pb* s, uint64_t arena_bytes, uint64_t small_limit, uint64_t batch)
{
	if (!s) return ABG_EINVAL;
	if (arena_bytes > PB_MAX_ARENA || (arena_bytes && arena_bytes < 4) || small_limit > abg::PB_SMALL_MAX || batch > (1ull << 24)) {
		s->error = "abg_pb_tune: an arena is 4 bytes to 2^40, small_limit at most 32, a batch at most 2^24 pairs";
		return ABG_EINVAL;
	}
	if (arena_bytes) s->arena_bytes = arena_bytes;
	if (small_limit) s->small_limit = small_limit;
	if (batch) s->batch = batch;
	return ABG_OK;
}

int abg_pb_align(abg_pb* s, uint64_t n, const uint8_t* a, const uint64_t* a_offsets, const uint8_t* b, const uint64_t* b_offsets, int want_consensus,
    uint32_t* matches, uint32_t* size, uint8_t* redone, uint64_t* cons_offsets, const uint8_t** cons)
{
	if (!s || !cons_offsets || !cons) return ABG_EINVAL;
	s->cons.clear();
	cons_offsets[0] = 0;
	*cons = s->cons.data();
	if (n == 0) return ABG_OK;
	if (!a_offsets || !b_offsets || !matches || !size || !redone || (a_offsets[n] && !a) || (b_offsets[n] && !b)) return ABG_EINVAL;
	if (!pb_offsets(s, a_offsets, n, "a_offsets") || !pb_offsets(s, b_offsets, n, "b_offsets")) return ABG_EINVAL;
	const uint64_t na = a_offsets[n], nb = b_offsets[n];
	if (!pb_valid(s, a, na, "a") || !pb_valid(s, b, nb, "b")) return ABG_EINVAL;
	(void)hipSetDevice(s->device);
	std::vector<uint8_t> in(na + nb);
	if (na) memcpy(in.data(), a, na);
	if (nb) memcpy(in.data() + na, b, nb);
	std::vector<PBPair> pairs(n);
	uint64_t cap = 0;
	for (uint64_t i = 0; i < n; ++i) {
		pairs[i] = PBPair{ a_offsets[i], na + b_offsets[i], 0, 0, cap, (uint32_t)(a_offsets[i + 1] - a_offsets[i]), (uint32_t)(b_offsets[i + 1] - b_offsets[i]), 0, 0 };
		cap += (uint64_t)pairs[i].la + pairs[i].lb;
	}
	hipError_t e = st::grow(&s->d_in, &s->in_cap, std::max<uint64_t>(in.size(), 64));
	if (e == hipSuccess && want_consensus) e = st::grow(&s->d_cons[0], &s->cons_cap[0], std::max<uint64_t>(cap, 64));
	if (e == hipSuccess && !in.empty()) e = hipMemcpyAsync(s->d_in, in.data(), in.size(), hipMemcpyHostToDevice, s->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
	if (e != hipSuccess) return st::fail(s->error, e, "uploading the pairs");
	const int rc = pb_run(s, pairs, in.data(), nullptr, want_consensus ? (uint8_t*)s->d_cons[0] : nullptr, matches, size, redone);
	if (rc != ABG_OK) return rc;
	if (want_consensus) {
		std::vector<uint8_t> all(cap);
		if (cap) e = hipMemcpy(all.data(), s->d_cons[0], cap, hipMemcpyDeviceToHost);
		if (e != hipSuccess) return st::fail(s->error, e, "fetching the consensuses");
		for (uint64_t i = 0; i < n; ++i) {
			const uint8_t* end = all.data() + pairs[i].cons_off + pairs[i].la + pairs[i].lb;
			s->cons.insert(s->cons.end(), end - size[i], end);
			cons_offsets[i + 1] = s->cons.size();
		}
	} else
		for (uint64_t i = 0; i < n; ++i) cons_offsets[i + 1] = 0;
	*cons = s->cons.data();
	return ABG_OK;
}

int abg_pb_align_chain(abg_pb* s, uint64_t ngroups, const uint64_t* group_first, const uint8_t* bytes, const uint64_t* offsets, uint32_t* matches, uint32_t* size,
    uint8_t* redone, uint64_t* cons_offsets, const uint8_t** cons)
{
	if (!s || !cons_offsets || !cons) return ABG_EINVAL;
	s->cons.clear();
	cons_offsets[0] = 0;
	*cons = s->cons.data();
	if (ngroups == 0) return ABG_OK;
	if (!group_first || !offsets || !matches || !size || !redone) return ABG_EINVAL;
	if (group_first[0] != 0) { s->error = "group_first[0] must be 0"; return ABG_EINVAL; }
	uint64_t rounds = 0;
	for (uint64_t g = 0; g < ngroups; ++g) {
		if (group_first[g + 1] < group_first[g] + 2) { s->error = "group " + std::to_string(g) + ": a group has two branches or more"; return ABG_EINVAL; }
		rounds = std::max(rounds, group_first[g + 1] - group_first[g] - 1);
	}
	const uint64_t nbranches = group_first[ngroups];
	if (!pb_offsets(s, offsets, nbranches, "offsets")) return ABG_EINVAL;
	const uint64_t total = offsets[nbranches];
	if ((total && !bytes) || !pb_valid(s, bytes, total, "bytes")) return ABG_EINVAL;
	(void)hipSetDevice(s->device);
	hipError_t e = st::grow(&s->d_in, &s->in_cap, std::max<uint64_t>(total, 64));
	if (e == hipSuccess && total) e = hipMemcpy(s->d_in, bytes, total, hipMemcpyHostToDevice);
	if (e != hipSuccess) return st::fail(s->error, e, "uploading the branches");
	// where each group's consensus of the round before starts, and its length; its matches so far
	std::vector<uint64_t> cur_off(ngroups);
	std::vector<uint32_t> cur_len(ngroups), acc(ngroups, 0), m, sz;
	std::vector<uint8_t> rd, all;
	std::vector<std::string> done(ngroups);
	std::vector<PBPair> pairs;
	std::vector<uint64_t> who;
	for (uint64_t g = 0; g < ngroups; ++g) redone[g] = 0;
	for (uint64_t r = 0; r < rounds; ++r) {
		pairs.clear();
		who.clear();
		uint64_t cap = 0;
		bool finishing = false;
		for (uint64_t g = 0; g < ngroups; ++g) {
			const uint64_t nb = group_first[g + 1] - group_first[g];
			if (nb < r + 2) continue;
			const uint64_t br = group_first[g] + r + 1;
			const uint32_t la = r == 0 ? (uint32_t)(offsets[group_first[g] + 1] - offsets[group_first[g]]) : cur_len[g], lb = (uint32_t)(offsets[br + 1] - offsets[br]);
			if ((uint64_t)la + lb > 0x3fffffffull) { s->error = "group " + std::to_string(g) + ": the consensus grows past 2^30 - 1 bytes"; return ABG_EINVAL; }
			pairs.push_back(PBPair{ r == 0 ? offsets[group_first[g]] : cur_off[g], offsets[br], 0, 0, cap, la, lb, r == 0 ? 0u : 1u, 0 });
			who.push_back(g);
			cap += (uint64_t)la + lb;
			finishing = finishing || nb == r + 2;
		}
		void*& out = s->d_cons[r & 1];
		e = st::grow(&out, &s->cons_cap[r & 1], std::max<uint64_t>(cap, 64));
		if (e != hipSuccess) return st::fail(s->error, e, "allocating a round");
		m.assign(pairs.size(), 0);
		sz.assign(pairs.size(), 0);
		rd.assign(pairs.size(), 0);
		const int rc = pb_run(s, pairs, bytes, (const uint8_t*)s->d_cons[(r & 1) ^ 1], (uint8_t*)out, m.data(), sz.data(), rd.data());
		if (rc != ABG_OK) return rc;
		if (finishing) {
			all.resize(cap);
			e = cap ? hipMemcpy(all.data(), out, cap, hipMemcpyDeviceToHost) : hipSuccess;
			if (e != hipSuccess) return st::fail(s->error, e, "fetching the consensuses");
		}
		for (size_t i = 0; i < pairs.size(); ++i) {
			const uint64_t g = who[i], nb = group_first[g + 1] - group_first[g];
			cur_len[g] = sz[i];
			cur_off[g] = pairs[i].cons_off + pairs[i].la + pairs[i].lb - sz[i];
			acc[g] = std::min(acc[g], m[i]); // alignMulti's min(matches, ...) from 0
			redone[g] = redone[g] || rd[i];
			if (nb == r + 2) {
				matches[g] = nb == 2 ? m[i] : acc[g];
				size[g] = sz[i];
				done[g].assign((const char*)all.data() + cur_off[g], sz[i]);
			}
		}
	}
	for (uint64_t g = 0; g < ngroups; ++g) {
		s->cons.insert(s->cons.end(), done[g].begin(), done[g].end());
		cons_offsets[g + 1] = s->cons.size();
	}
	*cons = s->cons.data();
	return ABG_OK;
}

int abg_pb_profile_get(abg_pb* s, const char* name, double* total_ms, uint64_t* launches)
{
	if (!s || !name) return ABG_EINVAL;
	(void)hipSetDevice(s->device);
	if (total_ms) *total_ms = 0;
	// not kernels: the pairs aligned on the host, the cells the kernels filled, the launches (one of each kernel at the most)
	if (!strcmp(name, "pb_redone")) { if (launches) *launches = s->redone; return ABG_OK; }
	if (!strcmp(name, "pb_cells")) { if (launches) *launches = s->cells; return ABG_OK; }
	if (!strcmp(name, "pb_launches")) { if (launches) *launches = s->launches; return ABG_OK; }
	return s->prof.get(name, total_ms, launches);
}

int abg_pb_profile_reset(abg_pb* s)
{
	if (!s) return ABG_EINVAL;
	(void)hipSetDevice(s->device);
	s->prof.clear();
	s->redone = s->cells = s->launches = 0;
	return ABG_OK;
}

} // extern "C"
