// abg_ov.hip -- Overlap's suffix/prefix search on the GPU and the abg_ov_* entry points (include/abyss_amd.h).
//
// ov_rc_kernel writes the reverse complement of every contig into the second half of the store, a thread a byte (the contig of a
// byte by binary search in the offsets).  ov_search_kernel gives a wavefront to a pair and runs abg::ov_search_pair (abg_ov.h):
// the lanes of a step read consecutive suffix positions of t, so their aligned words are shared in cache, and all of them read the
// same words of h.  abg_ov_find sorts the pairs by min(|t|, |h|), longest first, so the four waves of a workgroup and the
// workgroups of a launch finish together, and cuts the sorted list into launches of at most ABG_OV_BATCH_PAIRS pairs.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/abyss_amd.h"
#include "abg_ov.h"
#include "abg_stage.h"

namespace st = abg::stage;

static_assert(sizeof(abg_ov_pair) == sizeof(abg::OVPair), "ABI struct");

namespace {

__global__ __launch_bounds__(256) void ov_rc_kernel(uint8_t* __restrict__ store, const uint64_t* __restrict__ off, uint64_t n, uint64_t total)
{
	const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= total) return;
	uint64_t lo = 0, hi = n; // the last contig with off[c] <= i (empty contigs share an offset: take the one that holds byte i)
	while (hi - lo > 1) {
		const uint64_t mid = lo + (hi - lo) / 2;
		if (off[mid] <= i) lo = mid; else hi = mid;
	}
	const uint64_t a = off[lo], b = off[lo + 1];
	store[total + a + (b - 1 - i)] = abg::ov_complement(store[i]);
}

__global__ __launch_bounds__(abg::OV_BLOCK) void ov_search_kernel(const uint64_t* __restrict__ words, const abg::OVJob* __restrict__ jobs,
    uint32_t njobs, int mode, uint32_t* __restrict__ top3, uint32_t* __restrict__ ntop, uint64_t* __restrict__ bits)
{
	const uint32_t p = blockIdx.x * (abg::OV_BLOCK / abg::OV_WAVE) + threadIdx.x / abg::OV_WAVE;
	if (p >= njobs) return; // (a whole wave leaves together)
	const abg::OVJob j = jobs[p];
	abg::ov_search_pair(words, j, mode, top3 + 3 * (uint64_t)p, ntop + p, bits, (int)(threadIdx.x % abg::OV_WAVE));
}

} // namespace

struct abg_ov {
	int device = 0;
	hipStream_t stream = nullptr;
	uint64_t* words = nullptr; // the store: forward halves, reverse complements, OV_PAD zero bytes
	std::vector<uint64_t> off;  // n + 1 offsets
	uint64_t total = 0;
	uint64_t batch_pairs = 1ull << 20;
	void* din = nullptr; size_t in_cap = 0;
	void* dout = nullptr; size_t out_cap = 0;
	std::vector<uint32_t> all;      // the lengths of the last all-mode call
	std::vector<uint64_t> hbits;
	bool profiling = false;
	st::Profile prof;
	uint64_t bytes = 0; // suffix + prefix bytes of the pairs of the profiled calls
	std::string error;
	~abg_ov()
	{
		(void)hipSetDevice(device);
		if (stream) (void)hipStreamSynchronize(stream);
		prof.drop();
		if (words) (void)hipFree(words);
		if (din) (void)hipFree(din);
		if (dout) (void)hipFree(dout);
		if (stream) (void)hipStreamDestroy(stream);
	}
};

namespace {

std::string g_ov_create_error;

} // namespace

extern "C" {

int abg_ov_create(int device, abg_ov** out)
{
	if (!out) return ABG_EINVAL;
	*out = nullptr;
	hipStream_t stream = nullptr;
	const int rc = st::open_device(device, "overlap searcher", g_ov_create_error, &stream, 1);
	if (rc != ABG_OK) return rc;
	abg_ov* o = new abg_ov;
	o->device = device;
	o->stream = stream;
	if (const char* v = getenv("ABG_OV_BATCH_PAIRS")) {
		const unsigned long long t = strtoull(v, nullptr, 10);
		if (t > 0) o->batch_pairs = std::min<unsigned long long>(t, 1ull << 24);
	}
	*out = o;
	return ABG_OK;
}

void abg_ov_destroy(abg_ov* o) { delete o; }
const char* abg_ov_last_error(const abg_ov* o) { return o ? o->error.c_str() : g_ov_create_error.c_str(); }

int abg_ov_set_contigs(abg_ov* o, const uint8_t* bytes, const uint64_t* offsets, uint64_t n)
{
	if (!o || !offsets || (!bytes && n && offsets[n] != 0)) return ABG_EINVAL;
	if (n >= (1ull << 31)) { o->error = "at most 2^31 - 1 contigs"; return ABG_EINVAL; }
	if (offsets[0] != 0) { o->error = "offsets[0] must be 0"; return ABG_EINVAL; }
	for (uint64_t i = 0; i < n; ++i) {
		if (offsets[i + 1] < offsets[i] || offsets[i + 1] - offsets[i] > 0xFFFFFFFFull) {
			o->error = "contig " + std::to_string(i) + ": offsets must ascend and a contig has at most 2^32 - 1 bytes";
			return ABG_EINVAL;
		}
		for (uint64_t p = offsets[i]; p < offsets[i + 1]; ++p)
			if (abg::ov_complement(bytes[p]) == 0) { // where complementBaseChar asserts (Common/Sequence.cpp:41-44)
				char msg[96];
				snprintf(msg, sizeof msg, "contig %llu: unexpected character 0x%02x at position %llu", (unsigned long long)i, bytes[p],
				    (unsigned long long)(p - offsets[i]));
				o->error = msg;
				return ABG_EINVAL;
			}
	}
	(void)hipSetDevice(o->device);
	(void)hipStreamSynchronize(o->stream);
	if (o->words) (void)hipFree(o->words);
	o->words = nullptr;
	o->off.clear();
	o->total = 0;
	const uint64_t total = offsets[n];
	const uint64_t nbytes = ((2 * total + 7) & ~7ull) + abg::OV_PAD;
	uint64_t* doff = nullptr;
	hipError_t e = hipMalloc((void**)&o->words, nbytes);
	if (e == hipSuccess) e = hipMemsetAsync(o->words, 0, nbytes, o->stream);
	if (e == hipSuccess && total) e = hipMemcpyAsync(o->words, bytes, total, hipMemcpyHostToDevice, o->stream);
	if (e == hipSuccess && total) e = hipMalloc((void**)&doff, (n + 1) * 8);
	if (e == hipSuccess && total) e = hipMemcpyAsync(doff, offsets, (n + 1) * 8, hipMemcpyHostToDevice, o->stream);
	if (e == hipSuccess && total) {
		if ((total + 255) / 256 > 0x7FFFFFFFull) e = hipErrorInvalidValue;
		else {
			st::Timed t(o->prof, o->stream, "ov_rc", o->profiling);
			hipLaunchKernelGGL(ov_rc_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, o->stream, (uint8_t*)o->words, doff, n, total);
			e = hipGetLastError();
		}
	}
	if (e == hipSuccess) e = hipStreamSynchronize(o->stream);
	if (doff) (void)hipFree(doff);
	if (e != hipSuccess) {
		if (o->words) (void)hipFree(o->words);
		o->words = nullptr;
		return st::fail(o->error, e, "uploading the contigs");
	}
	o->off.assign(offsets, offsets + n + 1);
	o->total = total;
	return ABG_OK;
}

int abg_ov_find(abg_ov* o, const abg_ov_pair* pairs, uint64_t npairs, int mode, uint32_t* top3, uint32_t* ntop, uint64_t* all_offsets,
    const uint32_t** all)
{
	if (!o) return ABG_EINVAL;
	if (mode != abg::OV_TOP && mode != abg::OV_ALL) { o->error = "mode must be ABG_OV_TOP or ABG_OV_ALL"; return ABG_EINVAL; }
	if (mode == abg::OV_TOP ? (npairs && (!top3 || !ntop)) : (!all_offsets || !all)) return ABG_EINVAL;
	if (mode == abg::OV_ALL) { o->all.clear(); all_offsets[0] = 0; *all = o->all.data(); }
	if (npairs == 0) return ABG_OK;
	if (!pairs) return ABG_EINVAL;
	if (!o->words) { o->error = "no contigs have been set"; return ABG_EINVAL; }
	const uint64_t nn = 2 * (o->off.size() - 1);
	std::vector<abg::OVJob> jobs(npairs);
	for (uint64_t i = 0; i < npairs; ++i) {
		if (pairs[i].t >= nn || pairs[i].h >= nn) { o->error = "pair " + std::to_string(i) + ": no such contig"; return ABG_EINVAL; }
		const uint64_t t = pairs[i].t >> 1, h = pairs[i].h >> 1;
		jobs[i].tpos = (pairs[i].t & 1) * o->total + o->off[t];
		jobs[i].hpos = (pairs[i].h & 1) * o->total + o->off[h];
		jobs[i].tlen = (uint32_t)(o->off[t + 1] - o->off[t]);
		jobs[i].hlen = (uint32_t)(o->off[h + 1] - o->off[h]);
		jobs[i].bits = 0;
	}
	// longest first: the waves of a workgroup, and the workgroups of a launch, then carry like amounts of work
	std::vector<uint64_t> order(npairs);
	std::iota(order.begin(), order.end(), 0);
	auto work = [&](uint64_t i) { return std::min(jobs[i].tlen, jobs[i].hlen); };
	std::stable_sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) { return work(a) > work(b); });
	(void)hipSetDevice(o->device);
	std::vector<abg::OVJob> batch;
	std::vector<uint32_t> htop, hn;
	std::vector<std::vector<uint32_t>> found(mode == abg::OV_ALL ? npairs : 0);
	int rc = ABG_OK;
	for (uint64_t a = 0; a < npairs && rc == ABG_OK; a += o->batch_pairs) {
		const uint64_t b = std::min(npairs, a + o->batch_pairs), nb = b - a;
		batch.resize(nb);
		uint64_t nbits = 0;
		for (uint64_t i = 0; i < nb; ++i) {
			batch[i] = jobs[order[a + i]];
			batch[i].bits = nbits;
			if (mode == abg::OV_ALL) nbits += abg::ov_steps(batch[i].tlen, batch[i].hlen);
			if (o->profiling) o->bytes += 2ull * std::min(batch[i].tlen, batch[i].hlen);
		}
		const size_t out_bytes = mode == abg::OV_ALL ? (size_t)nbits * 8 : (size_t)nb * 16;
		hipError_t e = st::grow_slack(&o->din, &o->in_cap, nb * sizeof(abg::OVJob));
		if (e == hipSuccess) e = st::grow_slack(&o->dout, &o->out_cap, out_bytes + 8);
		if (e != hipSuccess) { rc = st::fail(o->error, e, "allocating a batch"); break; }
		e = hipMemcpyAsync(o->din, batch.data(), nb * sizeof(abg::OVJob), hipMemcpyHostToDevice, o->stream);
		if (e != hipSuccess) { rc = st::fail(o->error, e, "copying a batch to the device"); break; }
		uint32_t* dtop = (uint32_t*)o->dout;
		uint32_t* dn = dtop + 3 * nb;
		{
			st::Timed t(o->prof, o->stream, "ov_search", o->profiling);
			const unsigned per = abg::OV_BLOCK / abg::OV_WAVE;
			hipLaunchKernelGGL(ov_search_kernel, dim3((unsigned)((nb + per - 1) / per)), dim3(abg::OV_BLOCK), 0, o->stream, o->words,
			    (const abg::OVJob*)o->din, (uint32_t)nb, mode, dtop, dn, (uint64_t*)o->dout);
			e = hipGetLastError();
		}
		if (e != hipSuccess) { rc = st::fail(o->error, e, "launching the search"); break; }
		if (mode == abg::OV_TOP) {
			htop.resize(3 * nb); hn.resize(nb);
			e = hipMemcpyAsync(htop.data(), dtop, nb * 12, hipMemcpyDeviceToHost, o->stream);
			if (e == hipSuccess) e = hipMemcpyAsync(hn.data(), dn, nb * 4, hipMemcpyDeviceToHost, o->stream);
			if (e == hipSuccess) e = hipStreamSynchronize(o->stream);
			if (e != hipSuccess) { rc = st::fail(o->error, e, "the search"); break; }
			for (uint64_t i = 0; i < nb; ++i) {
				memcpy(top3 + 3 * order[a + i], htop.data() + 3 * i, 12);
				ntop[order[a + i]] = hn[i];
			}
		} else {
			o->hbits.resize(nbits);
			if (nbits) e = hipMemcpyAsync(o->hbits.data(), o->dout, nbits * 8, hipMemcpyDeviceToHost, o->stream);
			if (e == hipSuccess) e = hipStreamSynchronize(o->stream);
			if (e != hipSuccess) { rc = st::fail(o->error, e, "the search"); break; }
			for (uint64_t i = 0; i < nb; ++i) abg::ov_expand(o->hbits.data() + batch[i].bits, batch[i].tlen, batch[i].hlen, found[order[a + i]]);
		}
	}
	if (rc != ABG_OK) { (void)hipStreamSynchronize(o->stream); return rc; }
	if (mode == abg::OV_ALL) {
		for (uint64_t i = 0; i < npairs; ++i) {
			o->all.insert(o->all.end(), found[i].begin(), found[i].end());
			all_offsets[i + 1] = o->all.size();
		}
		*all = o->all.data();
	}
	return ABG_OK;
}

int abg_ov_profile(abg_ov* o, int on)
{
	if (!o) return ABG_EINVAL;
	o->profiling = on != 0;
	return ABG_OK;
}

int abg_ov_profile_get(abg_ov* o, const char* name, double* total_ms, uint64_t* launches)
{
	if (!o || !name) return ABG_EINVAL;
	(void)hipSetDevice(o->device);
	if (!strcmp(name, "ov_search_bytes")) { // not a kernel: 2 min(|t|, |h|) summed over the pairs of the profiled calls, as `launches`
		if (total_ms) *total_ms = 0;
		if (launches) *launches = o->bytes;
		return ABG_OK;
	}
	return o->prof.get(name, total_ms, launches);
}

} // extern "C"
