// abg_ov.h -- the suffix/prefix search of Overlap (bin/abyss-pe:658-659): which lengths l make the last l bytes of t the first l of h.
//
// Reference behaviour restated here (ABySS 2.3.10, paths relative to the repo):
//   Overlap/Overlap.cpp:145-149  sequence(node): the contig, or its reverse complement when the node's sense is set
//   Overlap/Overlap.cpp:159-166  for l = min(|t|, |h|) down to 1: t.substr(|t| - l, l) == h.substr(0, l) -> overlaps, descending
//   Overlap/Overlap.cpp:177-197  reads overlaps.empty(), overlaps[0..2] and size() >= 3 only: the three largest and how many exist
//   Overlap/Overlap.cpp:168-175  -v prints every overlap
//   Common/Sequence.cpp:21-45    the complement table: A C G T N . and the IUPAC codes, case kept; anything else asserts
//
// The store: the contigs' bytes end to end (case already folded by the reader, FastaReader::FOLD_CASE), then the reverse
// complement of each at the same offset of a second half, so node (id, sense) is the byte string at sense * total + offsets[id].
// Offsets are 64-bit.  The store is held as 64-bit words with OV_PAD zero bytes after it: ov_load8 builds the eight bytes at any
// byte position from two aligned words, so nothing depends on a wide load at an odd address, and a word that straddles the end of
// a string is masked to the bytes of the candidate before it is compared -- no byte outside the two strings of a pair takes part
// in a compare, which matters because the neighbour in a dense store is another contig, not a fault.
//
// The search: one wavefront a pair walks l downwards, 64 candidates a step, lane i holding l = top - i.  A lane compares a word
// at a time and leaves at its first differing word; on random sequence that is the first.  A 64-bit ballot collects a step's
// matches with bit i = candidate top - i, so ascending bits are descending lengths.  Top mode keeps the first three and stops
// there (they are the three largest); all mode stores every step's ballot, a bitmap the host expands.  ov_step is written once:
// the device takes the ballot across the wave, a host build runs the 64 lanes in a loop, and ov_search_pair is the same code.
#pragma once
#include "abg_core.h"
#include <cstdint>

namespace abg {

constexpr int OV_WAVE = 64;      // candidates a step
constexpr int OV_BLOCK = 256;    // four pairs a workgroup
constexpr uint64_t OV_PAD = 16;  // zero bytes after the store: ov_load8 reads the word after the one its position is in

enum { OV_TOP = 0, OV_ALL = 1 };

struct OVPair { uint32_t t, h; };  // abg_ov_pair of include/abyss_amd.h: oriented nodes, 2 * id + sense
// a pair as the kernel takes it: where the two strings are, and where its step ballots go in all mode
struct OVJob { uint64_t tpos, hpos; uint32_t tlen, hlen; uint64_t bits; };

// complementBaseChar (Common/Sequence.cpp:21-45); 0 where the reference asserts
ABG_HD uint8_t ov_complement(uint8_t c)
{
	const bool lower = c >= 'a' && c <= 'z';
	uint8_t rc;
	switch (lower ? c - 32 : c) {
	case 'A': rc = 'T'; break;
	case 'C': rc = 'G'; break;
	case 'G': rc = 'C'; break;
	case 'T': rc = 'A'; break;
	case 'N': rc = 'N'; break;
	case '.': rc = '.'; break;
	case 'M': rc = 'K'; break;
	case 'R': rc = 'Y'; break;
	case 'W': rc = 'W'; break;
	case 'S': rc = 'S'; break;
	case 'Y': rc = 'R'; break;
	case 'K': rc = 'M'; break;
	case 'V': rc = 'B'; break;
	case 'H': rc = 'D'; break;
	case 'D': rc = 'H'; break;
	case 'B': rc = 'V'; break;
	default: return 0;
	}
	return lower ? rc + 32 : rc;
}

// the eight bytes at byte position pos of the store, lowest address in the lowest byte
ABG_HD uint64_t ov_load8(const uint64_t* __restrict__ w, uint64_t pos)
{
	const uint64_t i = pos >> 3;
	const unsigned s = (unsigned)(pos & 7) * 8;
	const uint64_t lo = w[i];
	return s == 0 ? lo : (lo >> s) | (w[i + 1] << (64 - s));
}

// are the l bytes at a the l bytes at b?  (l >= 1)
ABG_HD bool ov_equal(const uint64_t* __restrict__ w, uint64_t a, uint64_t b, uint32_t l)
{
	for (uint32_t o = 0; o < l; o += 8) {
		uint64_t x = ov_load8(w, a + o) ^ ov_load8(w, b + o);
		const uint32_t rem = l - o;
		if (rem < 8) x &= (1ull << (rem * 8)) - 1;
		if (x) return false;
	}
	return true;
}

// one step: the candidates top, top - 1, ... top - 63 (those >= 1); bit i of the result says that top - i matches.
// On the device every lane of the wave calls this with its own lane and gets the same word.
ABG_HD uint64_t ov_step(const uint64_t* __restrict__ w, const OVJob& j, uint32_t top, int lane)
{
#if defined(__HIP_DEVICE_COMPILE__)
	const bool m = (uint32_t)lane < top && ov_equal(w, j.tpos + j.tlen - (top - lane), j.hpos, top - lane);
	return __ballot(m);
#else
	(void)lane;
	uint64_t b = 0;
	for (int i = 0; i < OV_WAVE && (uint32_t)i < top; ++i)
		if (ov_equal(w, j.tpos + j.tlen - (top - i), j.hpos, top - i)) b |= 1ull << i;
	return b;
#endif
}

ABG_HD int ov_ctz64(uint64_t x)
{
#if defined(__HIP_DEVICE_COMPILE__)
	return __ffsll((unsigned long long)x) - 1;
#else
	return __builtin_ctzll(x);
#endif
}

// steps a pair takes in all mode: the words of its bitmap
ABG_HD uint64_t ov_steps(uint32_t tlen, uint32_t hlen) { return ((uint64_t)(tlen < hlen ? tlen : hlen) + OV_WAVE - 1) / OV_WAVE; }

// The whole search of one pair.  Top mode: top3[0..2] the three largest matching lengths (zero-filled), *ntop how many exist.
// All mode: bits[j.bits + s] the ballot of step s, whose first candidate is min(|t|, |h|) - 64 s.  `lane` is the caller's lane on
// the device (lane 0 stores) and 0 on the host.
ABG_HD void ov_search_pair(const uint64_t* __restrict__ w, const OVJob& j, int mode, uint32_t* top3, uint32_t* ntop, uint64_t* bits, int lane)
{
	const uint32_t m = j.tlen < j.hlen ? j.tlen : j.hlen;
	uint32_t found[3] = { 0, 0, 0 };
	uint32_t n = 0;
	uint64_t s = 0;
	for (uint32_t top = m; top >= 1; top = top > OV_WAVE ? top - OV_WAVE : 0, ++s) {
		uint64_t b = ov_step(w, j, top, lane);
		if (mode == OV_ALL) {
			if (lane == 0) bits[j.bits + s] = b;
			continue;
		}
		while (b && n < 3) {
			found[n++] = top - (uint32_t)ov_ctz64(b);
			b &= b - 1;
		}
		if (n == 3) break;
	}
	if (mode == OV_TOP && lane == 0) {
		top3[0] = found[0]; top3[1] = found[1]; top3[2] = found[2];
		*ntop = n;
	}
}

// ---- host only from here

// every length in bits[0 .. ov_steps), descending, appended to out
template <class Vec> inline void ov_expand(const uint64_t* bits, uint32_t tlen, uint32_t hlen, Vec& out)
{
	uint32_t top = tlen < hlen ? tlen : hlen;
	for (uint64_t s = 0; top >= 1; top = top > OV_WAVE ? top - OV_WAVE : 0, ++s)
		for (uint64_t b = bits[s]; b; b &= b - 1) out.push_back(top - (uint32_t)__builtin_ctzll(b));
}

} // namespace abg
