// abg_kn.h -- the Konnector Bloom filter of `abyss-bloom build -t konnector` (the reference's default type), the file that
// abyss-sealer and konnector load with -i, and the probes of `abyss-bloom kmers`.
//
// Reference behaviour restated here:
//   Bloom/Bloom.h  Bloom::hash(key, seed)   CityHash64WithSeed over the canonical k-mer's packed bytes, (k + 3) / 4 of them
//   Common/Kmer.cpp                         packing: A C G T -> 0..3, four bases a byte, the first base in the high bits,
//                                           zero padding; canonical = the forward k-mer when it is <= its reverse complement
//                                           base by base (ties included, Kmer::isCanonical)
//   Common/city.cc                          CityHash64 v1.0 (2011): length classes 0-16, 17-32, 33-64 bytes (k <= 192 packs
//                                           into at most 48 bytes, so the >64-byte loop is never reached);
//                                           CityHash64WithSeed(s, n, seed) = HashLen16(CityHash64(s, n) - k2, seed)
//   Bloom/BloomFilter.h                     index = hash % bits; bit i is byte[i / 8] & (1 << (7 - i % 8))
//   Bloom/Bloom.h  loadSeq                  every window of k bases that is all ACGT is inserted
//   Bloom/CascadingBloomFilter.h            every level uses the same index; an insert sets the first level whose bit is clear
//   Bloom/BloomFilterWindow.h               a window [start, end] of the index space keeps only the indices inside it
//
// A k-mer lives in NW = ceil(k / 32) 64-bit words, big-endian: word j holds bases 32j .. 32j + 31, base 32j in bits 63..62.
// Its byte string (what CityHash reads) is therefore the words' big-endian serialisation, and a little-endian Fetch64 at byte
// offset o is bswap64 of the 64 bits that start at bit 8o of that string.
//
// Everything is ABG_HD: the kernels of abg_kn.hip are thin wrappers, and tests/hostcheck/kn_check.cc compiles the same
// functions with g++ for the CPU suite.
#pragma once
#include "abg_core.h"

namespace abg {

constexpr uint32_t KN_MAX_K = 192;
constexpr uint32_t KN_MAX_WORDS = 6; // ceil(192 / 32)
constexpr uint32_t KN_PAD = 256;     // 'N' bytes after a staged chunk: every window and word load of the last positions stays inside

struct KnParams {
	uint32_t k = 0, nw = 0, nbytes = 0, levels = 1;
	uint64_t seed = 0;
	uint64_t full_bits = 0;  // the index space: hash % full_bits
	Mod64 mod;               // ... as a divisor
	uint64_t start = 0, end = 0; // the window of the index space this filter holds, inclusive
	uint64_t level_words = 0;    // 32-bit words between two levels in device memory
};

inline KnParams make_kn_params(uint32_t k, uint64_t seed, uint64_t full_bits, uint32_t levels, uint64_t start, uint64_t end)
{
	KnParams p;
	p.k = k;
	p.nw = (k + 31) / 32;
	p.nbytes = (k + 3) / 4;
	p.levels = levels;
	p.seed = seed;
	p.full_bits = full_bits;
	p.mod = make_mod64(full_bits);
	p.start = start;
	p.end = end;
	const uint64_t bytes = (end - start + 1 + 7) / 8;
	p.level_words = (bytes + 15) / 16 * 4; // each level padded to 16 bytes (uint4 popcount loads)
	return p;
}

// A C G T of either case -> 0..3, anything else -> -1
ABG_HD int kn_code(unsigned c)
{
	const unsigned u = c & 0xDFu;
	const unsigned x = (u >> 1) & 3u; // A 0, C 1, T 2, G 3
	const bool ok = (u == 'A') | (u == 'C') | (u == 'G') | (u == 'T');
	return ok ? (int)(x ^ (x >> 1)) : -1;
}

ABG_HD uint64_t kn_bswap64(uint64_t x) { return __builtin_bswap64(x); }
ABG_HD uint32_t kn_bswap32(uint32_t x) { return __builtin_bswap32(x); }

// reverses the order of the 32 two-bit bases of a word
ABG_HD uint64_t kn_rev_bases(uint64_t x)
{
	x = ((x >> 2) & 0x3333333333333333ull) | ((x & 0x3333333333333333ull) << 2);
	x = ((x >> 4) & 0x0F0F0F0F0F0F0F0Full) | ((x & 0x0F0F0F0F0F0F0F0Full) << 4);
	return kn_bswap64(x);
}

template <int NW>
struct KnKmer {
	uint64_t w[NW];
};

// w[i] for a runtime i, 0 past the end; unrolled selects keep the words in registers
template <int NW>
ABG_HD uint64_t kn_word(const KnKmer<NW>& s, uint32_t i)
{
	uint64_t r = 0;
#pragma unroll
	for (int j = 0; j < NW; j++) r = i == (uint32_t)j ? s.w[j] : r;
	return r;
}

// the reverse complement of a k-mer: complement, reverse the padded string, then shift the (now leading) padding out
template <int NW>
ABG_HD KnKmer<NW> kn_revcomp(const KnKmer<NW>& f, uint32_t k)
{
	KnKmer<NW> r;
	const uint32_t pad = 64u * NW - 2u * k; // 0 .. 62
#pragma unroll
	for (int j = 0; j < NW; j++) r.w[j] = ~kn_rev_bases(f.w[NW - 1 - j]);
	if (pad) {
#pragma unroll
		for (int j = 0; j < NW; j++) r.w[j] = (r.w[j] << pad) | (j + 1 < NW ? r.w[j + 1] >> (64 - pad) : 0);
	}
	return r;
}

// Kmer::isCanonical: the forward k-mer is <= its reverse complement base by base (equal strings are canonical)
template <int NW>
ABG_HD bool kn_fwd_canonical(const KnKmer<NW>& f, const KnKmer<NW>& r)
{
	bool decided = false, fwd = true;
#pragma unroll
	for (int j = 0; j < NW; j++) {
		if (!decided && f.w[j] != r.w[j]) { decided = true; fwd = f.w[j] < r.w[j]; }
	}
	return fwd;
}

// ---- CityHash64 v1.0 over the packed bytes (lengths 1 .. 48) --------------------------------------------------------------
constexpr uint64_t CITY_K0 = 0xc3a5c85c97cb3127ull;
constexpr uint64_t CITY_K1 = 0xb492b66fbe98f273ull;
constexpr uint64_t CITY_K2 = 0x9ae16a3b2f90404full;
constexpr uint64_t CITY_K3 = 0xc949d7c7509e6557ull;
constexpr uint64_t CITY_MUL = 0x9ddfea08eb382d69ull;

ABG_HD uint64_t city_rot(uint64_t v, uint32_t s) { return s == 0 ? v : (v >> s) | (v << (64 - s)); }
ABG_HD uint64_t city_shift_mix(uint64_t v) { return v ^ (v >> 47); }
// Hash128to64 of the pair (low u, high v)
ABG_HD uint64_t city_len16(uint64_t u, uint64_t v)
{
	uint64_t a = (u ^ v) * CITY_MUL;
	a ^= a >> 47;
	uint64_t b = (v ^ a) * CITY_MUL;
	b ^= b >> 47;
	return b * CITY_MUL;
}

// 64 bits of the byte string from byte offset o on, in string order (byte o in the high byte)
template <int NW>
ABG_HD uint64_t kn_bits_at(const KnKmer<NW>& s, uint32_t o)
{
	const uint32_t m = o >> 3, sh = (o & 7u) * 8u;
	const uint64_t hi = kn_word(s, m);
	return sh ? (hi << sh) | (kn_word(s, m + 1) >> (64 - sh)) : hi;
}
template <int NW> ABG_HD uint64_t kn_fetch64(const KnKmer<NW>& s, uint32_t o) { return kn_bswap64(kn_bits_at(s, o)); }
template <int NW> ABG_HD uint64_t kn_fetch32(const KnKmer<NW>& s, uint32_t o) { return kn_bswap32((uint32_t)(kn_bits_at(s, o) >> 32)); }
template <int NW> ABG_HD uint64_t kn_byte(const KnKmer<NW>& s, uint32_t o) { return kn_bits_at(s, o) >> 56; }

template <int NW>
ABG_HD uint64_t city64(const KnKmer<NW>& s, uint32_t len)
{
	if (len <= 16) {
		if (len > 8) {
			const uint64_t a = kn_fetch64(s, 0), b = kn_fetch64(s, len - 8);
			return city_len16(a, city_rot(b + len, len)) ^ b;
		}
		if (len >= 4) {
			const uint64_t a = kn_fetch32(s, 0);
			return city_len16(len + (a << 3), kn_fetch32(s, len - 4));
		}
		const uint32_t y = (uint32_t)kn_byte(s, 0) + ((uint32_t)kn_byte(s, len >> 1) << 8);
		const uint32_t z = len + ((uint32_t)kn_byte(s, len - 1) << 2);
		return city_shift_mix((uint64_t)y * CITY_K2 ^ (uint64_t)z * CITY_K3) * CITY_K2;
	}
	if (len <= 32) {
		const uint64_t a = kn_fetch64(s, 0) * CITY_K1, b = kn_fetch64(s, 8);
		const uint64_t c = kn_fetch64(s, len - 8) * CITY_K2, d = kn_fetch64(s, len - 16) * CITY_K0;
		return city_len16(city_rot(a - b, 43) + city_rot(c, 30) + d, a + city_rot(b ^ CITY_K3, 20) - c + len);
	}
	// 33 .. 64
	uint64_t z = kn_fetch64(s, 24);
	uint64_t a = kn_fetch64(s, 0) + (len + kn_fetch64(s, len - 16)) * CITY_K0;
	uint64_t b = city_rot(a + z, 52), c = city_rot(a, 37);
	a += kn_fetch64(s, 8);
	c += city_rot(a, 7);
	a += kn_fetch64(s, 16);
	const uint64_t vf = a + z, vs = b + city_rot(a, 31) + c;
	a = kn_fetch64(s, 16) + kn_fetch64(s, len - 32);
	z = kn_fetch64(s, len - 8);
	b = city_rot(a + z, 52);
	c = city_rot(a, 37);
	a += kn_fetch64(s, len - 24);
	c += city_rot(a, 7);
	a += kn_fetch64(s, len - 16);
	const uint64_t wf = a + z, ws = b + city_rot(a, 31) + c;
	const uint64_t r = city_shift_mix((vf + ws) * CITY_K2 + (wf + vs) * CITY_K0);
	return city_shift_mix(r * CITY_K0 + vs) * CITY_K2;
}

template <int NW>
ABG_HD uint64_t city64_seed(const KnKmer<NW>& s, uint32_t len, uint64_t seed) { return city_len16(city64(s, len) - CITY_K2, seed); }

// Bloom::hash(key, seed): the hash of the canonical orientation of the forward k-mer f
template <int NW>
ABG_HD uint64_t kn_hash(const KnParams& p, const KnKmer<NW>& f)
{
	const KnKmer<NW> r = kn_revcomp(f, p.k);
	return kn_fwd_canonical(f, r) ? city64_seed(f, p.nbytes, p.seed) : city64_seed(r, p.nbytes, p.seed);
}

// ---- the staged stream: 2-bit codes (big-endian words of 32 bases) and a non-ACGT mask (bit j of word m: base 32m + j) ----

// codes and mask of the 32 characters c[0 .. 32)
template <class Get>
ABG_HD void kn_pack32(Get&& get, uint64_t& code, uint32_t& bad)
{
	code = 0;
	bad = 0;
	for (uint32_t j = 0; j < 32; j++) {
		const int c = kn_code(get(j));
		code = (code << 2) | (uint64_t)(c < 0 ? 0 : c);
		bad |= (uint32_t)(c < 0) << j;
	}
}

// the window [pos, pos + k) holds only ACGT (the mask is read, not the k characters)
ABG_HD bool kn_window_ok(const uint32_t* __restrict__ bad, uint64_t pos, uint32_t k)
{
	const uint64_t last = pos + k - 1;
	uint32_t any = 0;
	for (uint64_t m = pos >> 5; m <= (last >> 5); m++) {
		uint32_t w = bad[m];
		if (m == (pos >> 5)) w &= ~0u << (pos & 31);
		if (m == (last >> 5)) w &= ~0u >> (31 - (last & 31));
		any |= w;
	}
	return any == 0;
}

// the forward k-mer at pos, from the code words (NW + 1 of them are read from word pos / 32 on)
template <int NW>
ABG_HD KnKmer<NW> kn_extract(const uint64_t* __restrict__ codes, uint64_t pos, uint32_t k)
{
	KnKmer<NW> f;
	const uint64_t m = pos >> 5;
	const uint32_t sh = (uint32_t)(pos & 31) * 2;
	uint64_t cur = codes[m];
#pragma unroll
	for (int j = 0; j < NW; j++) {
		const uint64_t nxt = codes[m + j + 1];
		f.w[j] = sh ? (cur << sh) | (nxt >> (64 - sh)) : cur;
		cur = nxt;
	}
	const uint32_t tail = 2u * k - 64u * (NW - 1); // bits of the last word that belong to the k-mer: 2 .. 64
	if (tail < 64) f.w[NW - 1] &= ~0ull << (64 - tail);
	return f;
}

// the 32-bit word and mask of bit i of a level (byte i / 8, bit 7 - i % 8 of that byte; bytes little-endian in the word)
ABG_HD uint32_t kn_mask(uint64_t i) { return 1u << ((uint32_t)((i >> 3) & 3) * 8 + 7 - (uint32_t)(i & 7)); }

// the local bit of index idx in the window, or ~0 when the window does not hold it
ABG_HD uint64_t kn_local(const KnParams& p, uint64_t idx) { return idx < p.start || idx > p.end ? ~0ull : idx - p.start; }

// ---- host restatement: one k-mer at a time, as Bloom::loadSeq -------------------------------------------------------------

// the forward k-mer of the k ASCII characters s[0 .. k) (all ACGT)
template <int NW>
inline KnKmer<NW> kn_from_ascii(const char* s, uint32_t k)
{
	KnKmer<NW> f;
	for (int j = 0; j < NW; j++) f.w[j] = 0;
	for (uint32_t i = 0; i < k; i++) f.w[i >> 5] |= (uint64_t)kn_code((unsigned char)s[i]) << (62 - 2 * (i & 31));
	return f;
}

template <int NW>
inline uint64_t kn_hash_ascii_nw(const KnParams& p, const char* s) { return kn_hash<NW>(p, kn_from_ascii<NW>(s, p.k)); }

inline uint64_t kn_hash_ascii(const KnParams& p, const char* s)
{
	switch (p.nw) {
	case 1: return kn_hash_ascii_nw<1>(p, s);
	case 2: return kn_hash_ascii_nw<2>(p, s);
	case 3: return kn_hash_ascii_nw<3>(p, s);
	case 4: return kn_hash_ascii_nw<4>(p, s);
	case 5: return kn_hash_ascii_nw<5>(p, s);
	default: return kn_hash_ascii_nw<6>(p, s);
	}
}

// CascadingBloomFilter::insert on host arrays (levels[l]: the window's bytes of level l)
inline void kn_host_insert(const KnParams& p, uint8_t* const* levels, uint64_t idx)
{
	const uint64_t b = kn_local(p, idx);
	if (b == ~0ull) return;
	const uint8_t m = (uint8_t)(1u << (7 - (b & 7)));
	for (uint32_t l = 0; l < p.levels; l++) {
		if (!(levels[l][b >> 3] & m)) { levels[l][b >> 3] |= m; return; }
	}
}

// Bloom::loadSeq: every all-ACGT window of seq
template <class F>
inline void kn_host_windows(const KnParams& p, const char* seq, uint64_t len, F&& f)
{
	if (len < p.k) return;
	uint64_t run = 0;
	for (uint64_t i = 0; i < len; i++) {
		run = kn_code((unsigned char)seq[i]) < 0 ? 0 : run + 1;
		if (run >= p.k) f(i + 1 - p.k);
	}
}

} // namespace abg
