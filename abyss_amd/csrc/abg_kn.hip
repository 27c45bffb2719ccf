// abg_kn.hip -- gfx950 kernels and C ABI of the Konnector Bloom filter (include/abyss_amd.h, abg_kn_*; logic in abg_kn.h).
//
// A chunk of reads is staged as ASCII, one 'N' after every read (so no window spans two reads) and KN_PAD 'N's at the end.  A
// read longer than a staging slot goes as pieces that overlap by k - 1 characters (each window in exactly one piece).
//   k_kn_pack      one lane per 32 characters: two 16-byte loads, one 64-bit word of 2-bit codes and one 32-bit non-ACGT mask.
//                  Streaming: 1.375 bytes of HBM traffic per base.
//   k_kn_insert    one k-mer window per lane: the window's validity from the mask (at most 7 dwords, shared by neighbouring
//                  lanes through the cache), the forward k-mer from NW + 1 code words by funnel shifts, its reverse complement
//                  by bit tricks, the canonical one hashed (CityHash64WithSeed: ~10 64-bit multiplies, each several VALU
//                  instructions on CDNA, plus the byte gathers of the unaligned Fetch64s) and reduced % full_bits by a
//                  multiply-high.  Then the cascade as a chain of returning atomicOrs.  Bound: the hash is VALU work of a few
//                  hundred instructions per k-mer; the atomics are one random 4-byte RMW per k-mer, which moves a whole 64-byte
//                  sector once the filter is larger than the 256 MB Infinity Cache.  At 64 B of HBM per k-mer against ~6 TB/s
//                  the atomics allow ~90 G k-mers/s, far above what the hash leaves, so the kernel is VALU-bound in practice.
//   k_kn_contains  the same per-lane hash, then one load of the level instead of the atomics; a wave's 64 print flags go out as
//                  one ballot word.
//   k_kn_popcount  bits set per level (the statistics of bloom.cc printBloomStats / printCascadingBloomStats).
//
// Built with the rest of the library: hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -c
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/abyss_amd.h"
#include "abg_kn.h"
#include "abg_stage.h"

namespace st = abg::stage;

namespace {

__global__ void __launch_bounds__(256) k_kn_pack(const uint4* __restrict__ ascii, uint64_t nwords, uint64_t* __restrict__ codes,
    uint32_t* __restrict__ bad)
{
	uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
	for (; i < nwords; i += step) {
		const uint4 a = ascii[2 * i], b = ascii[2 * i + 1];
		const uint32_t d[8] = { a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w };
		uint64_t code;
		uint32_t m;
		abg::kn_pack32([&](uint32_t j) { return (d[j >> 2] >> (8 * (j & 3))) & 0xFFu; }, code, m);
		codes[i] = code;
		bad[i] = m;
	}
}

// Why the chain of returning atomicOrs is exact under any interleaving: for one index, each level's bit goes 0 -> 1 at most
// once, and the atomicOr that makes that transition (it returns the bit clear) is unique.  An insert moves on to level l + 1
// only after it saw level l's bit already set, so every level an insert claims has all the levels below it set at that moment.
// The claimed levels are therefore the first n clear ones (n = the inserts of that index, preset -L bits skipped), which is
// exactly what the reference's serial "set the first clear level" leaves behind, whatever the order.
template <int NW>
__global__ void __launch_bounds__(256) k_kn_insert(abg::KnParams p, const uint64_t* __restrict__ codes, const uint32_t* __restrict__ bad,
    uint64_t npos, uint32_t* __restrict__ levels)
{
	uint64_t pos = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
	for (; pos < npos; pos += step) {
		if (!abg::kn_window_ok(bad, pos, p.k)) continue;
		const uint64_t idx = abg::mod64(p.mod, abg::kn_hash<NW>(p, abg::kn_extract<NW>(codes, pos, p.k)));
		const uint64_t b = abg::kn_local(p, idx);
		if (b == ~0ull) continue;
		const uint32_t m = abg::kn_mask(b);
		uint32_t* w = levels + (b >> 5);
		for (uint32_t l = 0; l < p.levels; l++, w += p.level_words)
			if (!(atomicOr(w, m) & m)) break;
	}
}

// print[pos] = window pos is all ACGT and (its bit in level 0 is set) != inverse; bit pos % 64 of word pos / 64
template <int NW>
__global__ void __launch_bounds__(256) k_kn_contains(abg::KnParams p, const uint64_t* __restrict__ codes, const uint32_t* __restrict__ bad,
    uint64_t npos, const uint32_t* __restrict__ level, int inverse, unsigned long long* __restrict__ print)
{
	const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
	const uint64_t rounds = (npos + step - 1) / step; // every lane of a wave takes part in every ballot
	for (uint64_t r = 0; r < rounds; r++) {
		const uint64_t pos = r * step + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
		bool out = false;
		if (pos < npos && abg::kn_window_ok(bad, pos, p.k)) {
			const uint64_t idx = abg::mod64(p.mod, abg::kn_hash<NW>(p, abg::kn_extract<NW>(codes, pos, p.k)));
			const uint64_t b = abg::kn_local(p, idx);
			const bool in = b != ~0ull && (level[b >> 5] & abg::kn_mask(b)) != 0;
			out = in != (inverse != 0);
		}
		const unsigned long long word = __ballot(out);
		if ((threadIdx.x & 63) == 0 && pos < npos) print[pos >> 6] = word;
	}
}

__global__ void __launch_bounds__(256) k_kn_popcount(const uint4* __restrict__ words, uint64_t n16, unsigned long long* out)
{
	uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
	unsigned long long c = 0;
	for (; i < n16; i += step) {
		const uint4 v = words[i];
		c += __popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w);
	}
	for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o, 64);
	if ((threadIdx.x & 63) == 0 && c) atomicAdd(out, c);
}

// the hash, index and validity of every window of one sequence (known-answer tests)
template <int NW>
__global__ void __launch_bounds__(256) k_kn_hash(abg::KnParams p, const uint64_t* __restrict__ codes, const uint32_t* __restrict__ bad,
    uint64_t npos, unsigned long long* __restrict__ hash, unsigned long long* __restrict__ index, unsigned char* __restrict__ valid)
{
	uint64_t pos = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
	for (; pos < npos; pos += step) {
		const bool ok = abg::kn_window_ok(bad, pos, p.k);
		const uint64_t h = ok ? abg::kn_hash<NW>(p, abg::kn_extract<NW>(codes, pos, p.k)) : 0;
		hash[pos] = h;
		index[pos] = ok ? abg::mod64(p.mod, h) : 0;
		valid[pos] = ok;
	}
}

// A piece of the caller's sequences: `len` characters from seqs + at.  A sequence that does not fit a slot is cut into pieces
// that overlap by k - 1 characters, so that each of its windows lies in exactly one piece: a piece owns the windows that start
// at its first `own` positions (all of them for the last piece of a sequence, len - k + 1 for the others, whose last k - 1
// positions start the next piece).
struct Piece { uint64_t at, len, own; };

} // namespace

struct abg_kn {
	int device = 0;
	hipStream_t stream = nullptr;
	abg::KnParams p;
	uint64_t level_bits = 0, level_bytes = 0;
	uint32_t* levels = nullptr; // p.levels levels, p.level_words 32-bit words apart
	// two staging slots of `slot` bytes (pinned host memory the reads are packed into, device memory they are copied to, the event
	// that says the slot's kernels are done with both); the codes and the mask are shared: the kernels of one stream run one after
	// the other.  64 MiB; ABG_KN_SLOT_BYTES overrides it (tests: many slots and sequences cut into many pieces)
	size_t slot = 64u << 20;
	char* pin[2] = { nullptr, nullptr };
	char* dev[2] = { nullptr, nullptr };
	hipEvent_t done[2] = { nullptr, nullptr };
	bool busy[2] = { false, false };
	int next = 0;
	std::vector<Piece> staged; // the pieces of the chunk last staged, in order
	uint64_t* codes = nullptr;
	uint32_t* bad = nullptr;
	unsigned long long* aux = nullptr; size_t aux_cap = 0; // print flags / hash outputs
	unsigned long long* d_count = nullptr;
	uint32_t cus = 256;
	bool profiling = false;
	st::Profile prof;
	std::string error;
	~abg_kn()
	{
		(void)hipSetDevice(device);
		if (stream) (void)hipStreamSynchronize(stream);
		prof.drop();
		for (int i = 0; i < 2; i++) {
			if (pin[i]) (void)hipHostFree(pin[i]);
			if (dev[i]) (void)hipFree(dev[i]);
			if (done[i]) (void)hipEventDestroy(done[i]);
		}
		if (codes) (void)hipFree(codes);
		if (bad) (void)hipFree(bad);
		if (aux) (void)hipFree(aux);
		if (d_count) (void)hipFree(d_count);
		if (levels) (void)hipFree(levels);
		if (stream) (void)hipStreamDestroy(stream);
	}
};

namespace {

std::string g_kn_create_error;

// Staged bytes that fit a slot: each piece and its 'N', then padding up to a multiple of 32 plus KN_PAD (slot is a multiple of 32)
uint64_t slot_room(const abg_kn* f) { return f->slot - abg::KN_PAD - 32; }

// the next piece from the cursor (sequence i, character s of it) on; moves the cursor past what the piece owns
Piece next_piece(const uint64_t* off, uint64_t& i, uint64_t& s, uint64_t cap, uint32_t k)
{
	const uint64_t left = off[i + 1] - off[i] - s;
	Piece p{ off[i] + s, left, left };
	if (left > cap) {
		p.len = cap;
		p.own = cap - (k - 1);
		s += p.own;
	} else {
		i++;
		s = 0;
	}
	return p;
}

// pieces from the cursor on into dst as staged: piece, 'N', piece, 'N', ..., then 'N' up to a multiple of 32 plus KN_PAD, as
// many as fit a slot (at least one: no piece is longer than the room less its 'N'); f->staged lists them; returns the staged
// length before the padding
uint64_t stage(abg_kn* f, char* dst, const char* seqs, const uint64_t* off, uint64_t n, uint64_t& i, uint64_t& s)
{
	const uint64_t room = slot_room(f);
	f->staged.clear();
	uint64_t at = 0;
	while (i < n) {
		uint64_t ni = i, ns = s;
		const Piece p = next_piece(off, ni, ns, room - 1, f->p.k);
		if (at + p.len + 1 > room) break;
		memcpy(dst + at, seqs + p.at, p.len);
		dst[at + p.len] = 'N';
		at += p.len + 1;
		f->staged.push_back(p);
		i = ni;
		s = ns;
	}
	const uint64_t end = (at + 31) / 32 * 32 + abg::KN_PAD;
	memset(dst + at, 'N', end - at);
	return at;
}

unsigned grid_for(abg_kn* f, uint64_t n) { return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + 255) / 256, (uint64_t)f->cus * 16)); }

// codes and mask of a staged slot of `len` characters (+ padding)
int launch_pack(abg_kn* f, const char* dev, uint64_t len)
{
	st::Timed t(f->prof, f->stream, "kn_pack", f->profiling);
	const uint64_t nwords = (len + 31) / 32 + abg::KN_PAD / 32;
	k_kn_pack<<<grid_for(f, nwords), 256, 0, f->stream>>>((const uint4*)dev, nwords, f->codes, f->bad);
	const hipError_t e = hipGetLastError();
	return e == hipSuccess ? ABG_OK : st::fail(f->error, e, "the pack kernel launch");
}

#define KN_DISPATCH(NWV, CALL) \
	switch (NWV) { case 1: CALL(1); break; case 2: CALL(2); break; case 3: CALL(3); break; \
	               case 4: CALL(4); break; case 5: CALL(5); break; default: CALL(6); break; }

int launch_insert(abg_kn* f, uint64_t npos)
{
	st::Timed t(f->prof, f->stream, "kn_insert", f->profiling);
#define KN_INSERT(N) k_kn_insert<N><<<grid_for(f, npos), 256, 0, f->stream>>>(f->p, f->codes, f->bad, npos, f->levels)
	KN_DISPATCH(f->p.nw, KN_INSERT)
#undef KN_INSERT
	const hipError_t e = hipGetLastError();
	return e == hipSuccess ? ABG_OK : st::fail(f->error, e, "the insert kernel launch");
}

bool grow_aux(abg_kn* f, size_t bytes)
{
	if (bytes <= f->aux_cap) return true;
	if (f->aux) { (void)hipStreamSynchronize(f->stream); (void)hipFree(f->aux); f->aux = nullptr; f->aux_cap = 0; }
	const size_t cap = std::max<size_t>(bytes, 1u << 20);
	const hipError_t e = hipMalloc((void**)&f->aux, cap);
	if (e != hipSuccess) { (void)st::fail(f->error, e, "device memory for the results"); return false; }
	f->aux_cap = cap;
	return true;
}

// the staging slot s free for the host again
int wait_slot(abg_kn* f, int s)
{
	if (!f->busy[s]) return ABG_OK;
	const hipError_t e = hipEventSynchronize(f->done[s]);
	if (e != hipSuccess) return st::fail(f->error, e, "waiting for a staging slot");
	f->busy[s] = false;
	return ABG_OK;
}

// the pieces from the cursor on that fit slot s, staged into it, copied to the device and packed; *len: the staged length
int upload(abg_kn* f, int s, const char* seqs, const uint64_t* off, uint64_t n, uint64_t& i, uint64_t& c, uint64_t* len)
{
	int rc = wait_slot(f, s);
	if (rc != ABG_OK) return rc;
	*len = stage(f, f->pin[s], seqs, off, n, i, c);
	const uint64_t padded = (*len + 31) / 32 * 32 + abg::KN_PAD;
	hipError_t e = hipMemcpyAsync(f->dev[s], f->pin[s], padded, hipMemcpyHostToDevice, f->stream);
	if (e != hipSuccess) return st::fail(f->error, e, "copying reads to the device");
	return launch_pack(f, f->dev[s], *len);
}

} // namespace

extern "C" {

int abg_kn_create(int device, uint64_t full_bits, uint32_t levels, uint32_t k, uint64_t seed, uint64_t start, uint64_t end, abg_kn** out)
{
	if (!out) return ABG_EINVAL;
	*out = nullptr;
	if (full_bits == 0 || levels == 0 || k == 0 || k > abg::KN_MAX_K || start > end || end >= full_bits) {
		g_kn_create_error = "bad filter size, level count, k (1..192) or window";
		return ABG_EINVAL;
	}
	hipStream_t stream = nullptr;
	const int opened = st::open_device(device, "Konnector filter", g_kn_create_error, &stream, 1);
	if (opened != ABG_OK) return opened;
	abg_kn* f = new abg_kn;
	f->device = device;
	f->stream = stream;
	f->p = abg::make_kn_params(k, seed, full_bits, levels, start, end);
	f->level_bits = end - start + 1;
	f->level_bytes = (f->level_bits + 7) / 8;
	if (const char* v = getenv("ABG_KN_SLOT_BYTES")) f->slot = std::max<size_t>(1024, strtoull(v, nullptr, 10)) / 32 * 32; // (tests)
	hipDeviceProp_t prop;
	if (hipGetDeviceProperties(&prop, device) == hipSuccess) f->cus = (uint32_t)prop.multiProcessorCount;
	const size_t lbytes = (size_t)f->p.level_words * 4 * levels;
	const size_t words = f->slot / 32 + 16;
	hipError_t e = hipMalloc((void**)&f->levels, lbytes);
	if (e == hipSuccess) e = hipMemsetAsync(f->levels, 0, lbytes, f->stream);
	if (e == hipSuccess) e = hipMalloc((void**)&f->codes, words * 8);
	if (e == hipSuccess) e = hipMalloc((void**)&f->bad, words * 4);
	if (e == hipSuccess) e = hipMalloc((void**)&f->d_count, 8);
	for (int i = 0; i < 2 && e == hipSuccess; i++) {
		e = hipHostMalloc((void**)&f->pin[i], f->slot, hipHostMallocDefault);
		if (e == hipSuccess) e = hipMalloc((void**)&f->dev[i], f->slot);
		if (e == hipSuccess) e = hipEventCreateWithFlags(&f->done[i], hipEventDisableTiming);
	}
	if (e == hipSuccess) e = hipStreamSynchronize(f->stream);
	if (e != hipSuccess) {
		const int rc = st::create_fail(g_kn_create_error, e, "Konnector filter");
		delete f;
		return rc;
	}
	*out = f;
	return ABG_OK;
}

void abg_kn_destroy(abg_kn* f) { delete f; }
const char* abg_kn_last_error(const abg_kn* f) { return f ? f->error.c_str() : g_kn_create_error.c_str(); }

int abg_kn_import(abg_kn* f, uint32_t level, const uint8_t* bytes)
{
	if (!f || !bytes || level >= f->p.levels) return ABG_EINVAL;
	(void)hipSetDevice(f->device);
	hipError_t e = hipMemcpyAsync(f->levels + (size_t)level * f->p.level_words, bytes, f->level_bytes, hipMemcpyHostToDevice, f->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(f->stream);
	return e == hipSuccess ? ABG_OK : st::fail(f->error, e, "copying a level to the device");
}

int abg_kn_export(abg_kn* f, uint32_t level, uint8_t* bytes)
{
	if (!f || !bytes || level >= f->p.levels) return ABG_EINVAL;
	(void)hipSetDevice(f->device);
	hipError_t e = hipMemcpyAsync(bytes, f->levels + (size_t)level * f->p.level_words, f->level_bytes, hipMemcpyDeviceToHost, f->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(f->stream);
	return e == hipSuccess ? ABG_OK : st::fail(f->error, e, "copying a level to the host");
}

int abg_kn_insert_seqs(abg_kn* f, const char* seqs, const uint64_t* offsets, uint64_t n)
{
	if (!f || (n && (!seqs || !offsets))) return ABG_EINVAL;
	if (n == 0) return ABG_OK;
	(void)hipSetDevice(f->device);
	int rc = ABG_OK;
	for (uint64_t i = 0, c = 0; rc == ABG_OK && i < n;) {
		const int s = f->next;
		f->next ^= 1;
		uint64_t len = 0;
		rc = upload(f, s, seqs, offsets, n, i, c, &len);
		if (rc == ABG_OK) rc = launch_insert(f, len);
		if (rc == ABG_OK) {
			const hipError_t e = hipEventRecord(f->done[s], f->stream);
			if (e != hipSuccess) rc = st::fail(f->error, e, "hipEventRecord");
			else f->busy[s] = true;
		}
	}
	return rc;
}

int abg_kn_contains_seqs(abg_kn* f, const char* seqs, const uint64_t* offsets, uint64_t n, int inverse, uint8_t* print)
{
	if (!f || (n && (!seqs || !offsets || !print))) return ABG_EINVAL;
	if (n == 0) return ABG_OK;
	(void)hipSetDevice(f->device);
	int rc = ABG_OK;
	if (!grow_aux(f, (f->slot / 64 + 1) * 8)) rc = ABG_ENOMEM;
	std::vector<unsigned long long> bits;
	for (uint64_t i = 0, c = 0; rc == ABG_OK && i < n;) {
		const int s = f->next;
		f->next ^= 1;
		uint64_t len = 0;
		rc = upload(f, s, seqs, offsets, n, i, c, &len);
		if (rc != ABG_OK) break;
		{
			st::Timed t(f->prof, f->stream, "kn_contains", f->profiling);
			const unsigned grid = grid_for(f, len);
#define KN_CONTAINS(N) k_kn_contains<N><<<grid, 256, 0, f->stream>>>(f->p, f->codes, f->bad, len, f->levels, inverse, f->aux)
			KN_DISPATCH(f->p.nw, KN_CONTAINS)
#undef KN_CONTAINS
			const hipError_t e = hipGetLastError();
			if (e != hipSuccess) { rc = st::fail(f->error, e, "the probe kernel launch"); break; }
		}
		bits.resize((len + 63) / 64);
		hipError_t e = hipMemcpyAsync(bits.data(), f->aux, bits.size() * 8, hipMemcpyDeviceToHost, f->stream);
		if (e == hipSuccess) e = hipStreamSynchronize(f->stream);
		if (e != hipSuccess) { rc = st::fail(f->error, e, "reading the probes back"); break; }
		// staged position -> the caller's position: each piece's flags go to where it came from, up to the positions it owns
		// (the next piece writes the rest)
		uint64_t at = 0;
		for (const Piece& pc : f->staged) {
			uint8_t* dst = print + (pc.at - offsets[0]);
			for (uint64_t j = 0; j < pc.own; j++) dst[j] = (uint8_t)((bits[(at + j) >> 6] >> ((at + j) & 63)) & 1);
			at += pc.len + 1;
		}
	}
	return rc;
}

int abg_kn_popcount(abg_kn* f, uint64_t* per_level)
{
	if (!f || !per_level) return ABG_EINVAL;
	(void)hipSetDevice(f->device);
	for (uint32_t l = 0; l < f->p.levels; l++) {
		hipError_t e = hipMemsetAsync(f->d_count, 0, 8, f->stream);
		if (e == hipSuccess) {
			st::Timed t(f->prof, f->stream, "kn_popcount", f->profiling);
			const uint64_t n16 = f->p.level_words / 4;
			k_kn_popcount<<<grid_for(f, n16), 256, 0, f->stream>>>((const uint4*)(f->levels + (size_t)l * f->p.level_words), n16, f->d_count);
			e = hipGetLastError();
		}
		unsigned long long c = 0;
		if (e == hipSuccess) e = hipMemcpyAsync(&c, f->d_count, 8, hipMemcpyDeviceToHost, f->stream);
		if (e == hipSuccess) e = hipStreamSynchronize(f->stream);
		if (e != hipSuccess) return st::fail(f->error, e, "counting a level's bits");
		per_level[l] = c;
	}
	return ABG_OK;
}

int abg_kn_hash_seq(abg_kn* f, const char* seq, uint64_t len, uint64_t* hash, uint64_t* index, uint8_t* valid)
{
	if (!f || (len && (!seq || !hash || !index || !valid))) return ABG_EINVAL;
	if (len < f->p.k) return ABG_OK;
	if (len + 1 > slot_room(f)) { f->error = "abg_kn_hash_seq takes a sequence that fits one staging slot"; return ABG_EINVAL; }
	const uint64_t off[2] = { 0, len };
	(void)hipSetDevice(f->device);
	const uint64_t npos = len - f->p.k + 1;
	if (!grow_aux(f, npos * 17 + 16)) return ABG_ENOMEM;
	const int s = f->next;
	f->next ^= 1;
	uint64_t staged = 0, i = 0, c = 0;
	int rc = upload(f, s, seq, off, 1, i, c, &staged);
	if (rc != ABG_OK) return rc;
	unsigned long long* dh = f->aux;
	unsigned long long* di = f->aux + npos;
	unsigned char* dv = (unsigned char*)(f->aux + 2 * npos);
	{
		st::Timed t(f->prof, f->stream, "kn_hash", f->profiling);
#define KN_HASH(N) k_kn_hash<N><<<grid_for(f, npos), 256, 0, f->stream>>>(f->p, f->codes, f->bad, npos, dh, di, dv)
		KN_DISPATCH(f->p.nw, KN_HASH)
#undef KN_HASH
		const hipError_t e = hipGetLastError();
		if (e != hipSuccess) return st::fail(f->error, e, "the hash kernel launch");
	}
	hipError_t e = hipMemcpyAsync(hash, dh, npos * 8, hipMemcpyDeviceToHost, f->stream);
	if (e == hipSuccess) e = hipMemcpyAsync(index, di, npos * 8, hipMemcpyDeviceToHost, f->stream);
	if (e == hipSuccess) e = hipMemcpyAsync(valid, dv, npos, hipMemcpyDeviceToHost, f->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(f->stream);
	return e == hipSuccess ? ABG_OK : st::fail(f->error, e, "reading the hashes back");
}

int abg_kn_sync(abg_kn* f)
{
	if (!f) return ABG_EINVAL;
	(void)hipSetDevice(f->device);
	const hipError_t e = hipStreamSynchronize(f->stream);
	f->busy[0] = f->busy[1] = false;
	return e == hipSuccess ? ABG_OK : st::fail(f->error, e, "hipStreamSynchronize");
}

int abg_kn_profile(abg_kn* f, int on)
{
	if (!f) return ABG_EINVAL;
	f->profiling = on != 0;
	return ABG_OK;
}
int abg_kn_profile_get(abg_kn* f, const char* name, double* total_ms, uint64_t* launches)
{
	if (!f || !name) return ABG_EINVAL;
	(void)hipSetDevice(f->device);
	return f->prof.get(name, total_ms, launches);
}

} // extern "C"
