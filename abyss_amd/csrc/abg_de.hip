// abg_de.hip -- DistanceEst's scan over theta on the GPU and the abg_de_* entry points (include/abyss_amd.h).
//
// One workgroup takes up to DE_BLOCK consecutive thetas of one job, a lane each.  The PMF goes through LDS in tiles of DE_TILE
// entries; every lane reads the same entry (a broadcast).  The window's quotient depends on i - theta alone, so a workgroup fills
// a table of the DE_TILE + DE_BLOCK - 1 quotients a tile needs (one division each) and the inner loop reads it at consecutive
// addresses across lanes: two LDS reads, a multiply and a dependent add per term.  The sum of a lane runs over i = 0..maxValue in
// order whatever the tiling, so a PMF of any length takes this one path and gives the bits of abg::de_scan_job.
//
// This unit is compiled with -ffp-contract=off (abyss_amd/build.py): the device must not fuse pmf[i] * w into the add, and the
// host tail below must not either.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/abyss_amd.h"
#include "abg_de.h"
#include "abg_stage.h"

namespace st = abg::stage;

static_assert(sizeof(abg_de_job) == sizeof(abg::DEJob) && sizeof(abg_de_pair) == sizeof(abg::DEPair), "ABI structs");

namespace {

__global__ __launch_bounds__(abg::DE_BLOCK) void de_scan_kernel(const abg::DEJob* __restrict__ jobs, const uint2* __restrict__ blocks,
    const uint64_t* __restrict__ theta_off, const uint64_t* __restrict__ samp_off, const int32_t* __restrict__ sv,
    const uint32_t* __restrict__ sc, const double* __restrict__ pmf, const double* __restrict__ logp, int npmf, double minp,
    double logminp, double* __restrict__ c, double* __restrict__ like, uint32_t* __restrict__ n)
{
	__shared__ double s_p[abg::DE_TILE];
	__shared__ double s_w[abg::DE_TILE + abg::DE_BLOCK];
	const uint2 b = blocks[blockIdx.x]; // the job and the first theta of this workgroup, counted from the job's first
	const abg::DEJob j = jobs[b.x];
	const int B = (int)blockDim.x, lane = (int)threadIdx.x;
	const int64_t nth = (int64_t)j.last - j.first + 1;
	const int t0 = j.first + (int)b.y;
	const int theta = t0 + lane;
	const int x1 = (int)j.len0, x2 = (int)j.len1, x3 = (int)(j.len0 + j.len1);
	double cs = 0;
	for (int i0 = 0; i0 < npmf; i0 += abg::DE_TILE) {
		const int T = min(abg::DE_TILE, npmf - i0);
		__syncthreads();
		for (int q = lane; q < T; q += B) s_p[q] = pmf[i0 + q];
		// entry e holds window(x) for x = i0 - t0 - (B - 1) + e; lane l, entry q of the tile: x = i0 + q - t0 - l
		for (int e = lane; e < T + B - 1; e += B) s_w[e] = abg::de_window(i0 - t0 - (B - 1) + e, x1, x2, x3);
		__syncthreads();
		const double* w = s_w + (B - 1 - lane);
		for (int q = 0; q < T; ++q) cs = abg::de_c_term(cs, s_p[q], w[q]);
	}
	double lk = 0;
	unsigned cnt = 0;
	for (uint64_t s = samp_off[b.x]; s < samp_off[b.x + 1]; ++s)
		abg::de_like_step(lk, cnt, sv[s], sc[s], theta, pmf, logp, npmf, minp, logminp);
	if ((int64_t)b.y + lane < nth) {
		const uint64_t at = theta_off[b.x] + b.y + lane;
		c[at] = cs;
		like[at] = lk;
		n[at] = cnt;
	}
}

uint64_t align16(uint64_t x) { return (x + 15) & ~15ull; }

// one batch in flight: its inputs (pinned and on the device), its results (on the device and pinned)
struct Slot {
	void* hin = nullptr; void* din = nullptr; size_t in_cap = 0;
	void* hout = nullptr; void* dout = nullptr; size_t out_cap = 0;
	hipEvent_t done = nullptr;
	uint64_t thetas = 0;
};

} // namespace

struct abg_de {
	int device = 0;
	hipStream_t stream = nullptr;
	double* pmf = nullptr; double* logp = nullptr; // on the device
	int npmf = 0;
	double minp = 0, logminp = 0, mean = 0;
	uint64_t batch_thetas = 1ull << 20;
	uint32_t block = abg::DE_BLOCK;
	Slot slot[2];
	bool profiling = false;
	st::Profile prof;
	uint64_t terms = 0; // PMF entries x thetas of the profiled calls
	std::string error;
	~abg_de()
	{
		(void)hipSetDevice(device);
		if (stream) (void)hipStreamSynchronize(stream);
		prof.drop();
		for (Slot& s : slot) {
			if (s.hin) (void)hipHostFree(s.hin);
			if (s.din) (void)hipFree(s.din);
			if (s.hout) (void)hipHostFree(s.hout);
			if (s.dout) (void)hipFree(s.dout);
			if (s.done) (void)hipEventDestroy(s.done);
		}
		if (pmf) (void)hipFree(pmf);
		if (logp) (void)hipFree(logp);
		if (stream) (void)hipStreamDestroy(stream);
	}
};

namespace {

std::string g_de_create_error;

// Queues jobs [a, b) on slot s: inputs up, the kernel, results down into the slot's pinned buffer, the slot's event.
// The slot must be idle.  soff: the caller's sample offsets (njobs + 1).
int launch_batch(abg_de* d, Slot& s, const abg::DEJob* jobs, uint64_t a, uint64_t b, const int32_t* sv, const uint32_t* sc,
    const uint64_t* soff)
{
	const uint64_t nj = b - a, ns = soff[b] - soff[a];
	uint64_t thetas = 0, nblocks = 0;
	for (uint64_t i = a; i < b; ++i) {
		const uint64_t t = jobs[i].last < jobs[i].first ? 0 : (uint64_t)((int64_t)jobs[i].last - jobs[i].first + 1);
		thetas += t;
		nblocks += (t + d->block - 1) / d->block;
	}
	s.thetas = thetas;
	if (nblocks == 0) return ABG_OK;
	if (nblocks > 0x7FFFFFFFull) { d->error = "a batch has too many thetas"; return ABG_EINVAL; }
	const uint64_t o_jobs = 0, o_blocks = align16(o_jobs + nj * sizeof(abg::DEJob)), o_toff = align16(o_blocks + nblocks * 8),
	               o_soff = align16(o_toff + (nj + 1) * 8), o_sv = align16(o_soff + (nj + 1) * 8), o_sc = align16(o_sv + ns * 4),
	               in_bytes = align16(o_sc + ns * 4);
	const uint64_t o_c = 0, o_l = thetas * 8, o_n = thetas * 16, out_bytes = thetas * 20;
	hipError_t e = st::grow_pinned_slack(&s.hin, &s.din, &s.in_cap, in_bytes);
	if (e == hipSuccess) e = st::grow_pinned_slack(&s.hout, &s.dout, &s.out_cap, out_bytes);
	if (e != hipSuccess) return st::fail(d->error, e, "allocating a batch");
	char* h = (char*)s.hin;
	memcpy(h + o_jobs, jobs + a, nj * sizeof(abg::DEJob));
	uint2* blocks = (uint2*)(h + o_blocks);
	uint64_t* toff = (uint64_t*)(h + o_toff);
	uint64_t* so = (uint64_t*)(h + o_soff);
	uint64_t t_at = 0, b_at = 0;
	for (uint64_t i = 0; i < nj; ++i) {
		const abg::DEJob& j = jobs[a + i];
		const uint64_t t = j.last < j.first ? 0 : (uint64_t)((int64_t)j.last - j.first + 1);
		toff[i] = t_at;
		so[i] = soff[a + i] - soff[a];
		for (uint64_t q = 0; q < t; q += d->block) blocks[b_at++] = make_uint2((uint32_t)i, (uint32_t)q);
		t_at += t;
	}
	toff[nj] = t_at;
	so[nj] = ns;
	memcpy(h + o_sv, sv + soff[a], ns * 4);
	memcpy(h + o_sc, sc + soff[a], ns * 4);
	e = hipMemcpyAsync(s.din, s.hin, in_bytes, hipMemcpyHostToDevice, d->stream);
	if (e != hipSuccess) return st::fail(d->error, e, "copying a batch to the device");
	if (d->profiling) d->terms += thetas * (uint64_t)d->npmf;
	char* dv = (char*)s.din;
	char* dw = (char*)s.dout;
	{
		st::Timed t(d->prof, d->stream, "de_scan", d->profiling);
		hipLaunchKernelGGL(de_scan_kernel, dim3((unsigned)nblocks), dim3(d->block), 0, d->stream, (const abg::DEJob*)(dv + o_jobs),
		    (const uint2*)(dv + o_blocks), (const uint64_t*)(dv + o_toff), (const uint64_t*)(dv + o_soff), (const int32_t*)(dv + o_sv),
		    (const uint32_t*)(dv + o_sc), d->pmf, d->logp, d->npmf, d->minp, d->logminp, (double*)(dw + o_c), (double*)(dw + o_l),
		    (uint32_t*)(dw + o_n));
		e = hipGetLastError();
	}
	if (e != hipSuccess) return st::fail(d->error, e, "launching the scan");
	e = hipMemcpyAsync(s.hout, s.dout, out_bytes, hipMemcpyDeviceToHost, d->stream);
	if (e == hipSuccess) e = hipEventRecord(s.done, d->stream);
	if (e != hipSuccess) return st::fail(d->error, e, "copying a batch's results");
	return ABG_OK;
}

int wait_batch(abg_de* d, Slot& s)
{
	if (s.thetas == 0) return ABG_OK;
	const hipError_t e = hipEventSynchronize(s.done);
	return e == hipSuccess ? ABG_OK : st::fail(d->error, e, "the scan");
}

// where batches end: whole jobs, at most batch_thetas thetas unless one job alone has more
std::vector<uint64_t> cut_batches(const abg_de* d, const abg::DEJob* jobs, uint64_t n)
{
	std::vector<uint64_t> cuts{ 0 };
	uint64_t have = 0;
	for (uint64_t i = 0; i < n; ++i) {
		const uint64_t t = jobs[i].last < jobs[i].first ? 0 : (uint64_t)((int64_t)jobs[i].last - jobs[i].first + 1);
		if (have && have + t > d->batch_thetas) { cuts.push_back(i); have = 0; }
		have += t;
	}
	if (cuts.back() != n) cuts.push_back(n);
	return cuts;
}

int check_ready(abg_de* d)
{
	if (d->npmf == 0) { d->error = "no PMF has been set"; return ABG_EINVAL; }
	return ABG_OK;
}

int check_jobs(abg_de* d, const abg::DEJob* jobs, uint64_t n)
{
	for (uint64_t i = 0; i < n; ++i) {
		const abg::DEJob& j = jobs[i];
		if (j.last < j.first) continue;
		if (j.first < -abg::DE_RANGE || j.last > abg::DE_RANGE || j.len0 == 0 || j.len1 == 0 || j.len0 > j.len1 || (uint64_t)j.len0 + j.len1 > 0x7FFFFFFFull) {
			d->error = "a job is out of range (|theta| <= 2^29, 0 < len0 <= len1, len0 + len1 < 2^31)";
			return ABG_EINVAL;
		}
	}
	return ABG_OK;
}

} // namespace

extern "C" {

int abg_de_create(int device, abg_de** out)
{
	if (!out) return ABG_EINVAL;
	*out = nullptr;
	hipStream_t stream = nullptr;
	const int rc = st::open_device(device, "distance estimator", g_de_create_error, &stream, 1);
	if (rc != ABG_OK) return rc;
	abg_de* d = new abg_de;
	d->device = device;
	d->stream = stream;
	hipError_t e = hipSuccess;
	for (Slot& s : d->slot)
		if (e == hipSuccess) e = hipEventCreateWithFlags(&s.done, hipEventDisableTiming);
	if (e != hipSuccess) {
		const int failed = st::create_fail(g_de_create_error, e, "distance estimator");
		delete d;
		return failed;
	}
	if (const char* v = getenv("ABG_DE_BATCH_THETAS")) {
		const unsigned long long t = strtoull(v, nullptr, 10);
		if (t > 0) d->batch_thetas = t;
	}
	*out = d;
	return ABG_OK;
}

void abg_de_destroy(abg_de* d) { delete d; }
const char* abg_de_last_error(const abg_de* d) { return d ? d->error.c_str() : g_de_create_error.c_str(); }

int abg_de_set_pmf(abg_de* d, const double* pmf, uint64_t n, double minp, double mean)
{
	if (!d || !pmf) return ABG_EINVAL;
	if (n == 0 || n > (uint64_t)abg::DE_RANGE) { d->error = "the PMF must have 1 to 2^29 entries"; return ABG_EINVAL; }
	(void)hipSetDevice(d->device);
	(void)hipStreamSynchronize(d->stream);
	if (d->pmf) (void)hipFree(d->pmf);
	if (d->logp) (void)hipFree(d->logp);
	d->pmf = d->logp = nullptr;
	d->npmf = 0;
	std::vector<double> lp(n);
	for (uint64_t i = 0; i < n; ++i) lp[i] = log(pmf[i]);
	hipError_t e = hipMalloc((void**)&d->pmf, n * 8);
	if (e == hipSuccess) e = hipMalloc((void**)&d->logp, n * 8);
	if (e == hipSuccess) e = hipMemcpy(d->pmf, pmf, n * 8, hipMemcpyHostToDevice);
	if (e == hipSuccess) e = hipMemcpy(d->logp, lp.data(), n * 8, hipMemcpyHostToDevice);
	if (e != hipSuccess) return st::fail(d->error, e, "uploading the PMF");
	d->npmf = (int)n;
	d->minp = minp;
	d->logminp = log(minp);
	d->mean = mean;
	return ABG_OK;
}

int abg_de_tune(abg_de* d, uint32_t block_threads)
{
	if (!d) return ABG_EINVAL;
	if (block_threads == 0) block_threads = abg::DE_BLOCK;
	if (block_threads % 64 || block_threads > (uint32_t)abg::DE_BLOCK) { d->error = "the block must be 64, 128, 192 or 256 threads"; return ABG_EINVAL; }
	d->block = block_threads;
	return ABG_OK;
}

int abg_de_scan(abg_de* d, const abg_de_job* jobs_, uint64_t njobs, const int32_t* sv, const uint32_t* sc, const uint64_t* soff,
    double* c, double* like, uint32_t* n)
{
	if (!d) return ABG_EINVAL;
	if (njobs == 0) return ABG_OK;
	if (!jobs_ || !soff || !c || !like || !n || ((!sv || !sc) && soff[njobs] != soff[0])) return ABG_EINVAL;
	const abg::DEJob* jobs = (const abg::DEJob*)jobs_;
	int rc = check_ready(d);
	if (rc == ABG_OK) rc = check_jobs(d, jobs, njobs);
	if (rc != ABG_OK) return rc;
	if (soff[njobs] < soff[0]) return ABG_EINVAL;
	for (uint64_t s = soff[0]; s < soff[njobs]; ++s)
		if (sv[s] < -abg::DE_RANGE || sv[s] > abg::DE_RANGE) { d->error = "a sample value is out of range (|x| <= 2^29)"; return ABG_EINVAL; }
	(void)hipSetDevice(d->device);
	const std::vector<uint64_t> cuts = cut_batches(d, jobs, njobs);
	uint64_t at = 0;
	auto collect = [&](Slot& s) {
		const int r = wait_batch(d, s);
		if (r != ABG_OK) return r;
		const char* h = (const char*)s.hout;
		memcpy(c + at, h, s.thetas * 8);
		memcpy(like + at, h + s.thetas * 8, s.thetas * 8);
		memcpy(n + at, h + s.thetas * 16, s.thetas * 4);
		at += s.thetas;
		return (int)ABG_OK;
	};
	for (size_t b = 0; b + 1 < cuts.size() && rc == ABG_OK; ++b) {
		rc = launch_batch(d, d->slot[b & 1], jobs, cuts[b], cuts[b + 1], sv, sc, soff);
		if (rc == ABG_OK && b > 0) rc = collect(d->slot[(b - 1) & 1]);
	}
	if (rc == ABG_OK) rc = collect(d->slot[(cuts.size() - 2) & 1]);
	if (rc != ABG_OK) (void)hipStreamSynchronize(d->stream);
	return rc;
}

int abg_de_estimate(abg_de* d, const abg_de_pair* pairs_, uint64_t npairs, const int32_t* samples, const uint64_t* offsets,
    int32_t* distance, uint32_t* num_pairs)
{
	if (!d) return ABG_EINVAL;
	if (npairs == 0) return ABG_OK;
	if (!pairs_ || !samples || !offsets || !distance || !num_pairs) return ABG_EINVAL;
	int rc = check_ready(d);
	if (rc != ABG_OK) return rc;
	(void)hipSetDevice(d->device);
	const abg::DEPair* pairs = (const abg::DEPair*)pairs_;
	std::vector<abg::DEPrepared> prep(npairs);
	std::vector<abg::DEJob> jobs(npairs);
	std::vector<uint64_t> soff(npairs + 1, 0);
	for (uint64_t i = 0; i < npairs; ++i) {
		const char* why = abg::de_prepare(pairs[i], samples + offsets[i], offsets[i + 1] - offsets[i], d->npmf, d->mean, prep[i]);
		if (why) { d->error = std::string("pair ") + std::to_string(i) + ": " + why; return ABG_EINVAL; }
		jobs[i] = prep[i].job;
		soff[i + 1] = soff[i] + prep[i].values.size();
	}
	std::vector<int32_t> sv(soff[npairs]);
	std::vector<uint32_t> sc(soff[npairs]);
	for (uint64_t i = 0; i < npairs; ++i) {
		std::copy(prep[i].values.begin(), prep[i].values.end(), sv.begin() + soff[i]);
		std::copy(prep[i].counts.begin(), prep[i].counts.end(), sc.begin() + soff[i]);
	}
	const std::vector<double> hann = abg::de_hann(abg::de_filter_size(d->mean));
	const std::vector<uint64_t> cuts = cut_batches(d, jobs.data(), npairs);
	// the O(thetas) tail of a finished batch, on at most 16 host threads, while the device scans the next batch
	auto tail = [&](size_t b) {
		Slot& s = d->slot[b & 1];
		const int r = wait_batch(d, s);
		if (r != ABG_OK) return r;
		const char* h = (const char*)s.hout;
		const double* c = (const double*)h;
		const double* like = (const double*)(h + s.thetas * 8);
		const uint32_t* n = (const uint32_t*)(h + s.thetas * 16);
		std::vector<uint64_t> toff(cuts[b + 1] - cuts[b] + 1, 0);
		for (uint64_t i = cuts[b]; i < cuts[b + 1]; ++i) {
			const abg::DEJob& j = jobs[i];
			toff[i - cuts[b] + 1] = toff[i - cuts[b]] + (j.last < j.first ? 0 : (uint64_t)((int64_t)j.last - j.first + 1));
		}
		std::atomic<uint64_t> next(cuts[b]);
		auto work = [&]() {
			std::vector<double> le;
			for (uint64_t i; (i = next.fetch_add(1)) < cuts[b + 1];) {
				int theta;
				uint32_t bn;
				const uint64_t o = toff[i - cuts[b]];
				abg::de_tail(prep[i], hann, c + o, like + o, n + o, le, theta, bn);
				distance[i] = abg::de_finish(prep[i], theta);
				num_pairs[i] = bn;
			}
		};
		const uint64_t nj = cuts[b + 1] - cuts[b];
		unsigned nt = std::min<uint64_t>(16, std::max<uint64_t>(1, std::min<uint64_t>(nj / 8, std::thread::hardware_concurrency())));
		std::vector<std::thread> pool;
		for (unsigned t = 1; t < nt; ++t) pool.emplace_back(work);
		work();
		for (auto& t : pool) t.join();
		return (int)ABG_OK;
	};
	for (size_t b = 0; b + 1 < cuts.size() && rc == ABG_OK; ++b) {
		rc = launch_batch(d, d->slot[b & 1], jobs.data(), cuts[b], cuts[b + 1], sv.data(), sc.data(), soff.data());
		if (rc == ABG_OK && b > 0) rc = tail(b - 1);
	}
	if (rc == ABG_OK) rc = tail(cuts.size() - 2);
	if (rc != ABG_OK) (void)hipStreamSynchronize(d->stream);
	return rc;
}

int abg_de_profile(abg_de* d, int on)
{
	if (!d) return ABG_EINVAL;
	d->profiling = on != 0;
	return ABG_OK;
}

int abg_de_profile_get(abg_de* d, const char* name, double* total_ms, uint64_t* launches)
{
	if (!d || !name) return ABG_EINVAL;
	(void)hipSetDevice(d->device);
	if (!strcmp(name, "de_scan_terms")) { // not a kernel: PMF entries x thetas of the profiled calls, as `launches`
		if (total_ms) *total_ms = 0;
		if (launches) *launches = d->terms;
		return ABG_OK;
	}
	return d->prof.get(name, total_ms, launches);
}

} // extern "C"
