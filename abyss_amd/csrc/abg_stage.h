// abg_stage.h -- the host plumbing every stage unit (abg_rr.hip ... abg_mp.hip) shares: opening a device, the failure text and
// code of a HIP call, the event-timed launch profile behind abg_XX_profile_get, device buffers that grow, and the small parsers
// the tuning variables go through.  Host code only, and it needs the HIP runtime: nothing under csrc/host or tests/hostcheck
// includes it.  A unit keeps its own handle struct, kernels, entry points and counters ("What a stage unit consists of").
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../include/abyss_amd.h"

namespace abg {
namespace stage {

inline int code_of(hipError_t e) { return e == hipErrorOutOfMemory ? ABG_ENOMEM : ABG_EINTERNAL; }

// "<what> failed: <HIP's text>" into `error`; the ABI code of e.  Clears HIP's sticky last error.
inline int fail(std::string& error, hipError_t e, const char* what)
{
	(void)hipGetLastError();
	error = std::string(what) + " failed: " + hipGetErrorString(e);
	return code_of(e);
}

// a failure inside abg_XX_create, once the device is known to exist: "creating the <what> failed: ..."
inline int create_fail(std::string& create_error, hipError_t e, const char* what)
{
	return fail(create_error, e, (std::string("creating the ") + what).c_str());
}

// The head of every abg_XX_create: is there a device, is `device` one of them, make it current, create `nstreams` streams.
// On failure no stream is left behind, create_error says why and the ABI code comes back.
inline int open_device(int device, const char* what, std::string& create_error, hipStream_t* streams, int nstreams)
{
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
		(void)hipGetLastError();
		create_error = "no HIP device available (abyss_amd has no CPU fallback)";
		return ABG_ENODEV;
	}
	if (device < 0 || device >= n) { create_error = "HIP device ordinal out of range"; return ABG_ENODEV; }
	hipError_t e = hipSetDevice(device);
	int made = 0;
	for (; made < nstreams && e == hipSuccess; ++made) e = hipStreamCreate(&streams[made]);
	if (e == hipSuccess) return ABG_OK;
	for (int i = 0; i + 1 < made; ++i) (void)hipStreamDestroy(streams[i]); // (the last one counted is the one that failed)
	for (int i = 0; i < nstreams; ++i) streams[i] = nullptr;
	return create_fail(create_error, e, what);
}

// Milliseconds and launches per kernel name.  A launch is bracketed by two events (Timed) that wait in `pending` until somebody
// asks: drain() synchronises on them and adds them up.
struct Profile {
	struct Entry { double ms = 0; uint64_t launches = 0; };
	std::map<std::string, Entry> done;
	std::vector<std::pair<std::string, std::pair<hipEvent_t, hipEvent_t>>> pending;

	Profile() = default;
	Profile(const Profile&) = delete;
	Profile& operator=(const Profile&) = delete;
	~Profile() { drop(); }

	void drain()
	{
		for (auto& e : pending) {
			float ms = 0;
			(void)hipEventSynchronize(e.second.second);
			if (hipEventElapsedTime(&ms, e.second.first, e.second.second) == hipSuccess) { done[e.first].ms += ms; done[e.first].launches++; }
			(void)hipEventDestroy(e.second.first); (void)hipEventDestroy(e.second.second);
		}
		pending.clear();
	}
	// the stages that always time drain every n launches, so that events do not pile up over a long call
	void drain_if(size_t n) { if (pending.size() >= n) drain(); }
	void clear() { drain(); done.clear(); }
	// the pending events destroyed unread: what a handle's destructor does between synchronising its streams and freeing its memory
	void drop()
	{
		for (auto& e : pending) { (void)hipEventDestroy(e.second.first); (void)hipEventDestroy(e.second.second); }
		pending.clear();
	}
	// the tail of every abg_XX_profile_get, after the unit's own counters: a name never timed reads (0, 0)
	int get(const char* name, double* total_ms, uint64_t* launches)
	{
		drain();
		auto it = done.find(name);
		if (total_ms) *total_ms = it == done.end() ? 0 : it->second.ms;
		if (launches) *launches = it == done.end() ? 0 : it->second.launches;
		return ABG_OK;
	}
};

// Brackets the stream work of its scope with two events when `on`.  Read the launch error inside the scope: record, launch,
// hipGetLastError, record.
struct Timed {
	Profile& prof; hipStream_t stream; const char* name; hipEvent_t a = nullptr, b = nullptr;
	Timed(Profile& prof_, hipStream_t stream_, const char* name_, bool on = true) : prof(prof_), stream(stream_), name(name_)
	{
		if (!on) return;
		(void)hipEventCreate(&a); (void)hipEventCreate(&b);
		(void)hipEventRecord(a, stream);
	}
	Timed(const Timed&) = delete;
	Timed& operator=(const Timed&) = delete;
	~Timed()
	{
		if (!a) return;
		(void)hipEventRecord(b, stream);
		prof.pending.push_back({ name, { a, b } });
	}
};

// A device buffer of at least `need` bytes; what it held is lost when it grows.  Exact: the new capacity is `need`.
inline hipError_t grow(void** dev, size_t* cap, size_t need)
{
	if (need <= *cap) return hipSuccess;
	if (*dev) (void)hipFree(*dev);
	*dev = nullptr;
	*cap = 0;
	const hipError_t e = hipMalloc(dev, need);
	if (e == hipSuccess) *cap = need;
	return e;
}

// With slack, for buffers sized by the batch at hand (abg_ov, abg_de): a quarter more and a page, so a slightly larger batch fits
inline size_t with_slack(size_t need) { return need + need / 4 + 4096; }
inline hipError_t grow_slack(void** dev, size_t* cap, size_t need) { return need <= *cap ? hipSuccess : grow(dev, cap, with_slack(need)); }

// ... and a pinned host buffer and a device buffer of one size, grown together (abg_de's batch slots)
inline hipError_t grow_pinned_slack(void** host, void** dev, size_t* cap, size_t need)
{
	if (need <= *cap) return hipSuccess;
	if (*host) (void)hipHostFree(*host);
	if (*dev) (void)hipFree(*dev);
	*host = *dev = nullptr;
	*cap = 0;
	need = with_slack(need);
	hipError_t e = hipHostMalloc(host, need);
	if (e == hipSuccess) e = hipMalloc(dev, need);
	if (e == hipSuccess) *cap = need;
	return e;
}

// a tuning variable: unset or empty gives dflt, anything else is clamped to [lo, hi]
inline unsigned long long env_u64(const char* name, unsigned long long lo, unsigned long long hi, unsigned long long dflt)
{
	const char* v = getenv(name);
	if (!v || !*v) return dflt;
	const unsigned long long t = strtoull(v, nullptr, 10);
	return std::max(lo, std::min(hi, t));
}

inline size_t up(size_t x, size_t a) { return (x + a - 1) / a * a; }

} // namespace stage
} // namespace abg
