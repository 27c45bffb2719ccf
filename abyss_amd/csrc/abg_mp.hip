// abg_mp.hip -- abyss-mergepairs' overlap alignment on the GPU and the abg_mp_* entry points (include/abyss_amd.h).
//
// One kernel, a wave a pair (abg_mp.h has the cell, the selection and the filters it shares with the host):
//   mp_wave_kernel  Both reads go to LDS first, read 2 reversed and complemented through the host's 256-byte table.  Rows go in
//                   stripes of 64, lane l holding row i0 + l + 1, and the wave sweeps anti-diagonals: at step t lane l is at column
//                   t - l + 1.  The cell above (score, matches | length << 16, start | fail) and its column's character come from
//                   lane l - 1 by a cross-lane move; the left and diagonal neighbours are the lane's own registers.  Lane 0's row
//                   above is the previous stripe's last row, kept in LDS as three arrays of dwords: the wave loads 64 columns of it
//                   at a time and lane 0 takes its column by a uniform cross-lane read; the lane that holds a stripe's last row
//                   stores its cells there, never ahead of the loads (a column is loaded at or before the step that stores it).
//                   isMatch is a bit of the host's 256 x 256 table: a lane keeps the 128 bits of its row's character in four
//                   registers, so a cell's score costs no memory access.  After the last stripe the buffer holds the last row; the
//                   64 lanes take every 64th column of it through mp_select and reduce over the wave, and lane 0 writes the record.
//                   For an order-dependent pair the wave claims lb cells of the spill arena with one atomic add and stores the row
//                   there for the host's std::sort (mp_replay); where the arena is full the record says so and the host sends the
//                   pair out again.
// The kernel's limit is MP_KERNEL_MAX = 512 bases a read: the three arrays of the row buffer and the two reads then take 7 KB of
// LDS, which leaves room for more than twenty waves a CU, matches and length of any path (at most 1,024 cells) share a dword, and
// every read a sequencer of paired short reads writes is well inside it.  A longer read, or a byte of 128 and above (the lane's
// four registers hold the table's first 128 columns), sends the pair to the host's mp_align_host, the same header.
// Batches of ABG_MP_BATCH pairs alternate between two streams, each with buffers of its own, so a batch's upload and download run
// beside the other's kernel.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/abyss_amd.h"
#include "abg_mp.h"
#include "abg_stage.h"

namespace st = abg::stage;

static_assert(sizeof(abg_mp_record) == sizeof(abg::MPRecord), "abg_mp_record is MPRecord");

namespace {

using abg::MPCell;
using abg::MPPair;
using abg::MPRecord;

constexpr uint32_t KMAX = abg::MP_KERNEL_MAX;

// the row buffer in LDS, as mp_select reads it
struct LdsRow {
	const int* h; const uint32_t* ml; const uint32_t* st;
	__device__ MPCell operator[](uint32_t j) const { const uint32_t x = ml[j]; return MPCell{ h[j], x & 0xffff, x >> 16, st[j] }; }
};

// the kernel's lanes in mp_select
struct MPWave {
	uint32_t lane;
	__device__ uint32_t first() const { return lane; }
	__device__ uint32_t step() const { return 64; }
	__device__ bool any(bool x) const { return __ballot(x) != 0; }
	__device__ int max(int x) const { for (int o = 32; o; o >>= 1) { const int y = __shfl_xor(x, o); x = y > x ? y : x; } return x; }
	__device__ uint32_t sum(uint32_t x) const { for (int o = 32; o; o >>= 1) x += (uint32_t)__shfl_xor((int)x, o); return x; }
};

__global__ __launch_bounds__(64) void mp_wave_kernel(const MPPair* __restrict__ pairs, const uint8_t* __restrict__ in, const uint32_t* __restrict__ table,
    const uint8_t* __restrict__ comp, const uint32_t* __restrict__ min_identity, uint32_t min_matches, MPRecord* __restrict__ records, MPCell* __restrict__ spill,
    unsigned long long spill_cells, unsigned long long* __restrict__ spill_used)
{
	__shared__ uint8_t sa[KMAX], sb[KMAX];
	__shared__ int row_h[KMAX];
	__shared__ uint32_t row_ml[KMAX], row_st[KMAX];
	const MPPair p = pairs[blockIdx.x];
	const uint32_t la = p.la, lb = p.lb, lane = threadIdx.x;
	if (la > KMAX || lb > KMAX) { // (the host keeps such a pair: nothing here may index past the buffers)
		if (lane == 0) records[blockIdx.x] = MPRecord{ 0, 0, 0, 0, 0, 0, 0, 0, abg::MP_TOO_LONG, 0 };
		return;
	}
	for (uint32_t k = lane; k < la; k += 64) sa[k] = in[p.a_off + k];
	for (uint32_t k = lane; k < lb; k += 64) sb[k] = comp[in[p.b_off + (lb - 1 - k)]];
	__syncthreads();
	for (uint32_t i0 = 0; i0 < la; i0 += 64) {
		const uint32_t i = i0 + lane + 1, nlive = la - i0 < 64 ? la - i0 : 64, writer = nlive - 1;
		const bool live = i <= la;
		const uint32_t ca = live ? sa[i - 1] & 127u : 0;
		const uint4 bits = *(const uint4*)(table + ca * 8);
		MPCell diag = abg::mp_column0(), left = abg::mp_column0();
		int mine_h = 0, line_h = 0;
		uint32_t mine_ml = 0, mine_st = 0, line_ml = 0, line_st = 0, cb = 0, cb_line = 0;
		const uint32_t steps = lb + nlive - 1;
		for (uint32_t t = 0; t < steps; t++) {
			if ((t & 63) == 0) { // the next 64 columns: their characters, and the row above them
				const uint32_t c = t + lane;
				cb_line = c < lb ? sb[c] : 0;
				if (i0 > 0 && c < lb) { line_h = row_h[c]; line_ml = row_ml[c]; line_st = row_st[c]; }
			}
			int up_h = __shfl_up(mine_h, 1);
			uint32_t up_ml = (uint32_t)__shfl_up((int)mine_ml, 1), up_st = (uint32_t)__shfl_up((int)mine_st, 1);
			const uint32_t cb_up = (uint32_t)__shfl_up((int)cb, 1);
			const int src = (int)(t & 63);
			const int l_h = __shfl(line_h, src);
			const uint32_t l_ml = (uint32_t)__shfl((int)line_ml, src), l_st = (uint32_t)__shfl((int)line_st, src), cb_new = (uint32_t)__shfl((int)cb_line, src);
			if (lane == 0) {
				up_h = i0 == 0 ? abg::MP_NEG : l_h;
				up_ml = i0 == 0 ? 0 : l_ml;
				up_st = i0 == 0 ? 0 : l_st;
				cb = cb_new;
			} else
				cb = cb_up;
			const int j = (int)t - (int)lane + 1;
			if (live && j >= 1 && j <= (int)lb) {
				const uint32_t k = (cb >> 5) & 3, word = k == 0 ? bits.x : k == 1 ? bits.y : k == 2 ? bits.z : bits.w;
				const MPCell up = MPCell{ up_h, up_ml & 0xffff, up_ml >> 16, up_st };
				const MPCell cell = abg::mp_cell(diag, up, left, (word >> (cb & 31)) & 1, i, (uint32_t)j);
				diag = up;
				left = cell;
				mine_h = cell.h;
				mine_ml = cell.matches | cell.length << 16;
				mine_st = cell.start;
				if (lane == writer) { row_h[j - 1] = mine_h; row_ml[j - 1] = mine_ml; row_st[j - 1] = mine_st; }
			}
		}
		__syncthreads(); // the row buffer, for the next stripe and for the selection
	}
	const LdsRow row{ row_h, row_ml, row_st };
	MPRecord r;
	abg::mp_select(row, la, lb, min_matches, min_identity, r, MPWave{ lane });
	if (r.flags & abg::MP_ORDER_DEPENDENT) {
		unsigned long long base = 0;
		if (lane == 0) base = atomicAdd(spill_used, (unsigned long long)lb);
		base = ((unsigned long long)(uint32_t)__shfl((int)(base >> 32), 0) << 32) | (uint32_t)__shfl((int)(uint32_t)base, 0);
		if (base + lb <= spill_cells) {
			for (uint32_t j = lane; j < lb; j += 64) spill[base + j] = row[j];
			r.spill = (uint32_t)base;
		} else
			r.flags |= abg::MP_UNSPILLED;
	}
	if (lane == 0) records[blockIdx.x] = r;
}

struct Slot { // a stream and what a batch in flight on it owns
	hipStream_t stream = nullptr;
	void* d_in = nullptr; size_t in_cap = 0;
	void* d_meta = nullptr; size_t meta_cap = 0; // pairs, records, the arena's counter
	void* d_spill = nullptr; size_t spill_cap = 0;
	std::vector<uint8_t> in;
	std::vector<MPPair> pairs;
	std::vector<uint64_t> ids;
	std::vector<MPRecord> recs;
	unsigned long long used = 0;
	size_t rec_at = 0, used_at = 0;
	bool busy = false;
};

} // namespace

struct abg_mp {
	int device = 0;
	Slot slot[2];
	uint64_t max_len = abg::MP_KERNEL_MAX, spill_bytes = 64ull << 20, batch = 1ull << 16;
	void* d_tables = nullptr; // the match table, the complement table, min_identity
	float table_identity = 0;
	bool tables_ready = false;
	st::Profile prof;
	uint64_t spilled = 0, host_run = 0, cells = 0, launches = 0, relaunched = 0;
	std::string error;
	~abg_mp()
	{
		(void)hipSetDevice(device);
		for (Slot& s : slot)
			if (s.stream) (void)hipStreamSynchronize(s.stream);
		prof.drop();
		for (Slot& s : slot) {
			for (void* p : { s.d_in, s.d_meta, s.d_spill })
				if (p) (void)hipFree(p);
			if (s.stream) (void)hipStreamDestroy(s.stream);
		}
		if (d_tables) (void)hipFree(d_tables);
	}
};

namespace {

std::string g_mp_create_error;

constexpr size_t TABLE_AT = 0, COMP_AT = 256 * 8 * 4, IDENTITY_AT = COMP_AT + 256, IDENTITY_N = 2 * KMAX + 1, TABLES_BYTES = IDENTITY_AT + IDENTITY_N * 4;
constexpr uint64_t MP_MAX_SPILL = 1ull << 35, MP_MAX_BATCH = 1ull << 24;

// the three tables of a call: the first two once, min_identity whenever the identity changes
int mp_tables(abg_mp* s, float identity)
{
	hipError_t e = hipSuccess;
	if (!s->d_tables) e = hipMalloc(&s->d_tables, TABLES_BYTES);
	if (e != hipSuccess) return st::fail(s->error, e, "allocating the tables");
	if (s->tables_ready && memcmp(&identity, &s->table_identity, sizeof identity) == 0) return ABG_OK;
	for (Slot& q : s->slot) // (a kernel of the call before may still read them)
		if ((e = hipStreamSynchronize(q.stream)) != hipSuccess) return st::fail(s->error, e, "waiting for a stream");
	std::vector<uint8_t> host(TABLES_BYTES);
	const std::vector<uint32_t> table = abg::mp_match_table(), ident = abg::mp_identity_table(identity, (uint32_t)IDENTITY_N - 1);
	memcpy(host.data() + TABLE_AT, table.data(), 256 * 8 * 4);
	for (int c = 0; c < 256; ++c) host[COMP_AT + c] = abg::ov_complement((uint8_t)c);
	memcpy(host.data() + IDENTITY_AT, ident.data(), IDENTITY_N * 4);
	e = hipMemcpy(s->d_tables, host.data(), TABLES_BYTES, hipMemcpyHostToDevice);
	if (e != hipSuccess) return st::fail(s->error, e, "uploading the tables");
	s->tables_ready = true;
	s->table_identity = identity;
	return ABG_OK;
}

struct Call { // one abg_mp_align
	const uint8_t* a; const uint64_t* a_off; const uint8_t* b; const uint64_t* b_off;
	uint32_t min_matches; const uint32_t* min_identity; // (the host's table, for the replay and the host's pairs)
	MPRecord* out;
	std::vector<uint64_t> again; // pairs whose row found no room in the arena
};

std::string read_of(const uint8_t* bytes, const uint64_t* off, uint64_t i) { return std::string((const char*)bytes + off[i], (size_t)(off[i + 1] - off[i])); }

void host_pair(abg_mp* s, Call& c, uint64_t id)
{
	abg::mp_align_host(read_of(c.a, c.a_off, id), abg::mp_reverse_complement(read_of(c.b, c.b_off, id)), c.min_matches, c.min_identity, c.out[id]);
	c.out[id].flags |= abg::MP_TOO_LONG;
	s->host_run++;
}

// Queues the pairs ids[0 .. n) on a slot: upload, kernel, download of the records and of the arena's counter
int mp_launch(abg_mp* s, Slot& q, Call& c, const uint64_t* ids, uint64_t n)
{
	q.in.clear();
	q.pairs.resize(n);
	q.ids.assign(ids, ids + n);
	for (uint64_t k = 0; k < n; ++k) {
		const uint64_t id = ids[k], la = c.a_off[id + 1] - c.a_off[id], lb = c.b_off[id + 1] - c.b_off[id];
		q.pairs[k] = MPPair{ q.in.size(), q.in.size() + la, (uint32_t)la, (uint32_t)lb };
		q.in.insert(q.in.end(), c.a + c.a_off[id], c.a + c.a_off[id + 1]);
		q.in.insert(q.in.end(), c.b + c.b_off[id], c.b + c.b_off[id + 1]);
		s->cells += la * lb;
	}
	const unsigned long long spill_cells = s->spill_bytes / sizeof(MPCell);
	q.rec_at = st::up(n * sizeof(MPPair), 64);
	q.used_at = q.rec_at + st::up(n * sizeof(MPRecord), 64);
	hipError_t e = st::grow(&q.d_in, &q.in_cap, std::max<size_t>(q.in.size(), 64));
	if (e == hipSuccess) e = st::grow(&q.d_meta, &q.meta_cap, q.used_at + 64);
	if (e == hipSuccess) e = st::grow(&q.d_spill, &q.spill_cap, std::max<size_t>(spill_cells * sizeof(MPCell), 64));
	if (e != hipSuccess) return st::fail(s->error, e, "allocating a launch");
	char* meta = (char*)q.d_meta;
	if (!q.in.empty()) e = hipMemcpyAsync(q.d_in, q.in.data(), q.in.size(), hipMemcpyHostToDevice, q.stream);
	if (e == hipSuccess) e = hipMemcpyAsync(meta, q.pairs.data(), n * sizeof(MPPair), hipMemcpyHostToDevice, q.stream);
	if (e == hipSuccess) e = hipMemsetAsync(meta + q.used_at, 0, 8, q.stream);
	if (e != hipSuccess) return st::fail(s->error, e, "copying a launch to the device");
	const char* tables = (const char*)s->d_tables;
	{
		st::Timed t(s->prof, q.stream, "mp_wave");
		hipLaunchKernelGGL(mp_wave_kernel, dim3((unsigned)n), dim3(64), 0, q.stream, (const MPPair*)meta, (const uint8_t*)q.d_in, (const uint32_t*)(tables + TABLE_AT),
		    (const uint8_t*)(tables + COMP_AT), (const uint32_t*)(tables + IDENTITY_AT), c.min_matches, (MPRecord*)(meta + q.rec_at), (MPCell*)q.d_spill, spill_cells,
		    (unsigned long long*)(meta + q.used_at));
		e = hipGetLastError();
	}
	if (e != hipSuccess) return st::fail(s->error, e, "launching the alignment");
	q.recs.resize(n);
	e = hipMemcpyAsync(q.recs.data(), meta + q.rec_at, n * sizeof(MPRecord), hipMemcpyDeviceToHost, q.stream);
	if (e == hipSuccess) e = hipMemcpyAsync(&q.used, meta + q.used_at, 8, hipMemcpyDeviceToHost, q.stream);
	if (e != hipSuccess) return st::fail(s->error, e, "queueing the download");
	q.busy = true;
	s->launches++;
	return ABG_OK;
}

// Waits for a slot's batch and finishes its records: the rows of the order-dependent pairs come back and are replayed
int mp_collect(abg_mp* s, Slot& q, Call& c)
{
	if (!q.busy) return ABG_OK;
	q.busy = false;
	hipError_t e = hipStreamSynchronize(q.stream);
	if (e != hipSuccess) return st::fail(s->error, e, "the alignment");
	const unsigned long long spill_cells = s->spill_bytes / sizeof(MPCell), filled = std::min(q.used, spill_cells);
	std::vector<MPCell> rows((size_t)filled);
	if (filled) {
		e = hipMemcpy(rows.data(), q.d_spill, (size_t)filled * sizeof(MPCell), hipMemcpyDeviceToHost);
		if (e != hipSuccess) return st::fail(s->error, e, "fetching the spilled rows");
	}
	for (size_t k = 0; k < q.recs.size(); ++k) {
		const uint64_t id = q.ids[k];
		MPRecord r = q.recs[k];
		if (r.flags & abg::MP_TOO_LONG) { s->error = "a pair past the kernel's limit reached the kernel"; return ABG_EINTERNAL; }
		if (r.flags & abg::MP_UNSPILLED) {
			if ((unsigned long long)q.pairs[k].lb > spill_cells) host_pair(s, c, id); // no arena of this size ever holds its row
			else c.again.push_back(id);
			continue;
		}
		if (r.flags & abg::MP_ORDER_DEPENDENT) {
			if ((unsigned long long)r.spill + q.pairs[k].lb > filled) { s->error = "a spilled row lies outside the arena"; return ABG_EINTERNAL; }
			abg::mp_replay(rows.data() + r.spill, q.pairs[k].la, q.pairs[k].lb, c.min_matches, c.min_identity, r);
			r.flags |= abg::MP_ORDER_DEPENDENT;
			s->spilled++;
		}
		r.spill = 0;
		c.out[id] = r;
	}
	s->prof.drain_if(64);
	return ABG_OK;
}

// ids through the two slots in batches, each collected when its slot comes up again
int mp_run(abg_mp* s, Call& c, const std::vector<uint64_t>& ids)
{
	unsigned turn = 0;
	for (uint64_t at = 0; at < ids.size(); at += s->batch, turn ^= 1) {
		Slot& q = s->slot[turn];
		int rc = mp_collect(s, q, c);
		if (rc == ABG_OK) rc = mp_launch(s, q, c, ids.data() + at, std::min<uint64_t>(s->batch, ids.size() - at));
		if (rc != ABG_OK) return rc;
	}
	for (unsigned k = 0; k < 2; ++k, turn ^= 1) {
		const int rc = mp_collect(s, s->slot[turn], c);
		if (rc != ABG_OK) return rc;
	}
	return ABG_OK;
}

bool mp_offsets(abg_mp* s, const uint64_t* off, uint64_t n, const char* what)
{
	if (off[0] != 0) { s->error = std::string(what) + "[0] must be 0"; return false; }
	for (uint64_t i = 0; i < n; ++i)
		if (off[i + 1] < off[i] || off[i + 1] - off[i] > abg::MP_MAX_READ) { s->error = std::string(what) + " must ascend, a read at most 100,000 bytes"; return false; }
	return true;
}

} // namespace

extern "C" {

int abg_mp_create(int device, abg_mp** out)
{
	if (!out) return ABG_EINVAL;
	*out = nullptr;
	hipStream_t stream[2] = { nullptr, nullptr };
	const int rc = st::open_device(device, "pair aligner", g_mp_create_error, stream, 2);
	if (rc != ABG_OK) return rc;
	abg_mp* s = new abg_mp;
	s->device = device;
	for (int i = 0; i < 2; ++i) s->slot[i].stream = stream[i];
	s->max_len = st::env_u64("ABG_MP_MAX_LEN", 1, abg::MP_KERNEL_MAX, s->max_len);
	s->spill_bytes = st::env_u64("ABG_MP_SPILL_BYTES", sizeof(MPCell), MP_MAX_SPILL, s->spill_bytes);
	s->batch = st::env_u64("ABG_MP_BATCH", 1, MP_MAX_BATCH, s->batch);
	*out = s;
	return ABG_OK;
}

void abg_mp_destroy(abg_mp* s) { delete s; }
const char* abg_mp_last_error(const abg_mp* s) { return s ? s->error.c_str() : g_mp_create_error.c_str(); }

int abg_mp_tune(abg_mp* s, uint64_t max_len, uint64_t spill_bytes, uint64_t batch)
{
	if (!s) return ABG_EINVAL;
	if (max_len > abg::MP_KERNEL_MAX || spill_bytes > MP_MAX_SPILL || (spill_bytes && spill_bytes < sizeof(MPCell)) || batch > MP_MAX_BATCH) {
		s->error = "abg_mp_tune: max_len is at most 512, a spill arena 16 bytes to 2^35, a batch at most 2^24 pairs";
		return ABG_EINVAL;
	}
	if (max_len) s->max_len = max_len;
	if (spill_bytes) s->spill_bytes = spill_bytes;
	if (batch) s->batch = batch;
	return ABG_OK;
}

int abg_mp_align(abg_mp* s, uint64_t n, const uint8_t* a, const uint64_t* a_offsets, const uint8_t* b, const uint64_t* b_offsets, uint32_t min_matches, float identity,
    abg_mp_record* records)
{
	if (!s) return ABG_EINVAL;
	if (n == 0) return ABG_OK;
	if (!a_offsets || !b_offsets || !records || (a_offsets[n] && !a) || (b_offsets[n] && !b)) return ABG_EINVAL;
	if (!mp_offsets(s, a_offsets, n, "a_offsets") || !mp_offsets(s, b_offsets, n, "b_offsets")) return ABG_EINVAL;
	for (uint64_t p = 0; p < b_offsets[n]; ++p)
		if (!abg::ov_complement(b[p])) { s->error = "b: byte " + std::to_string(p) + " has no complement"; return ABG_EINVAL; }
	(void)hipSetDevice(s->device);
	int rc = mp_tables(s, identity);
	if (rc != ABG_OK) return rc;
	uint32_t longest = 0;
	for (uint64_t i = 0; i < n; ++i) longest = std::max<uint32_t>(longest, (uint32_t)(a_offsets[i + 1] - a_offsets[i] + b_offsets[i + 1] - b_offsets[i]));
	const std::vector<uint32_t> min_identity = abg::mp_identity_table(identity, longest);
	Call c{ a, a_offsets, b, b_offsets, min_matches, min_identity.data(), (MPRecord*)records, {} };
	// which pairs the kernel takes
	std::vector<uint64_t> ids;
	ids.reserve(n);
	for (uint64_t i = 0; i < n; ++i) {
		const uint64_t la = a_offsets[i + 1] - a_offsets[i], lb = b_offsets[i + 1] - b_offsets[i];
		bool device = la <= s->max_len && lb <= s->max_len;
		for (uint64_t p = a_offsets[i]; device && p < a_offsets[i + 1]; ++p) device = a[p] < 128;
		for (uint64_t p = b_offsets[i]; device && p < b_offsets[i + 1]; ++p) device = b[p] < 128;
		if (device) ids.push_back(i);
		else host_pair(s, c, i);
	}
	while (!ids.empty()) {
		rc = mp_run(s, c, ids);
		if (rc != ABG_OK) return rc;
		s->relaunched += c.again.size();
		ids.swap(c.again); // the pairs whose rows found the arena full: again, with the arena to themselves
		c.again.clear();
	}
	return ABG_OK;
}

int abg_mp_profile_get(abg_mp* s, const char* name, double* total_ms, uint64_t* launches)
{
	if (!s || !name) return ABG_EINVAL;
	(void)hipSetDevice(s->device);
	if (total_ms) *total_ms = 0;
	// not kernels: the pairs whose rows the host sorted, the pairs the host aligned, the cells the kernel filled, the batches, the
	// pairs sent out again because the arena was full
	if (!strcmp(name, "mp_spilled")) { if (launches) *launches = s->spilled; return ABG_OK; }
	if (!strcmp(name, "mp_host")) { if (launches) *launches = s->host_run; return ABG_OK; }
	if (!strcmp(name, "mp_cells")) { if (launches) *launches = s->cells; return ABG_OK; }
	if (!strcmp(name, "mp_launches")) { if (launches) *launches = s->launches; return ABG_OK; }
	if (!strcmp(name, "mp_relaunched")) { if (launches) *launches = s->relaunched; return ABG_OK; }
	return s->prof.get(name, total_ms, launches);
}

int abg_mp_profile_reset(abg_mp* s)
{
	if (!s) return ABG_EINVAL;
	(void)hipSetDevice(s->device);
	s->prof.clear();
	s->spilled = s->host_run = s->cells = s->launches = s->relaunched = 0;
	return ABG_OK;
}

} // extern "C"
