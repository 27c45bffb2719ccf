// abg_pb.h -- the global alignment of PopBubbles (bin/abyss-pe:604-605): matches, consensus length and consensus of two branches.
//
// Reference behaviour restated here (ABySS 2.3.10, paths relative to the repo):
//   Align/alignGlobal.cc:20-29     MATCH 5, MISMATCH -4, GAP_OPEN -12, GAP_EXTEND -4
//   Align/alignGlobal.cc:35-44     score(a, b, c): equal characters match with c = a; otherwise c = ambiguityOr(a, b) and it is a
//                                  match when c is one of the two (Common/Sequence.h:102-107, restated as mc_detail::ambiguity)
//   Align/alignGlobal.cc:158-183   the boundaries and the cell: g from above, h from the left, f the best of diagonal, g and h
//   Align/alignGlobal.cc:57-136    backtrack: diagonal first, then vertical with its run loop, then horizontal, then the tails
//   Align/alignGlobal.h:47-69      alignPair returns (matches, consensus size); alignMulti chains the consensus through the branches
//
// What is kept of the three matrices: five bits a cell.  backtrack compares, at cell (i, j),
//   PB_DIAG  f == f[i-1][j-1] + s
//   PB_VERT  f == f[i-1][j] + OPEN || f == g[i-1][j] + EXTEND.  g[i][j] is the larger of those two terms and f >= g[i][j], so f
//            equals one of them exactly when f == g[i][j]: if f equals a term, g <= f is at least that term, so g == f; and g is
//            one of its terms.  (No sum wraps: INT_MIN / 2 only ever takes one OPEN or EXTEND, the maximum drops it at once.)
//   PB_HORZ  f == h[i][j], by the same argument
//   PB_VEXT  g[i][j] == g[i-1][j] + EXTEND, the run loop's test: the run goes on upwards
//   PB_HEXT  h[i][j] == h[i][j-1] + EXTEND
// and nothing else, so a cell's byte of flags replays it.  Row i of a pair's flags is at (i - 1) * pb_stride(|b|): rows are padded
// to four bytes so that a lane of the wave kernel stores four cells as one word.
//
// pb_cell and pb_traceback are the text the host and both kernels (abg_pb.hip) compile.  pb_score is the reference's; the wave
// kernel scores from pb_code, five bits a character, which pb_check proves equal to it on every pair of codes.
#pragma once
#include "abg_mc.h"

#include <climits>
#include <cstdint>
#include <string>
#include <vector>

namespace abg {

constexpr int PB_MATCH = 5, PB_MISMATCH = -4, PB_GAP_OPEN = -12, PB_GAP_EXTEND = -4, PB_NEG = INT_MIN / 2;
constexpr uint32_t PB_SMALL_MAX = 32;  // the longest side a lane takes on its own: its two rows live in LDS
enum { PB_DIAG = 1, PB_VERT = 2, PB_HORZ = 4, PB_VEXT = 8, PB_HEXT = 16 };

// a pair as the kernels take it: a at a_off of the input bytes (a_src 0) or of the previous round's consensuses (a_src 1), b at
// b_off of the input bytes, flags at flag_off of the arena, the row buffer at row_off (wave kernel), the consensus ending at
// cons_off + la + lb of the output
struct PBPair { uint64_t a_off, b_off, flag_off, row_off, cons_off; uint32_t la, lb, a_src, pad; };

ABG_HD uint64_t pb_stride(uint32_t lb) { return ((uint64_t)lb + 3) & ~(uint64_t)3; }
ABG_HD uint64_t pb_cells(uint32_t la, uint32_t lb) { return (uint64_t)la * pb_stride(lb); }
// f[n][0] = g[n][0], f[0][n] = h[0][n]
ABG_HD int pb_edge(uint32_t n) { return n == 0 ? 0 : PB_GAP_OPEN + PB_GAP_EXTEND * ((int)n - 1); }

ABG_HD int pb_score(uint8_t a, uint8_t b, uint8_t& c)
{
	if (a == b) { c = a; return PB_MATCH; }
	c = (uint8_t)mc_detail::ambiguity((char)a, (char)b, true);
	return c == a || c == b ? PB_MATCH : PB_MISMATCH;
}

// a character as the wave kernel carries it: its mask, and 16 when it is lowercase; 0 for a byte ambiguityToBitmask asserts on
ABG_HD uint32_t pb_code(uint8_t c)
{
	const unsigned m = mc_mask(mc_upper(c));
	return m == 0 ? 0 : m | (mc_lower(c) ? 16u : 0u);
}
// score(a, b) == MATCH from the codes.  c = ambiguityOr(a, b) is the code of the masks' union, lowercase when either is; it is a
// again when b's mask adds nothing to a's and the case is a's (a lowercase, or b not), and likewise b.  a == b is the case where
// both hold.
ABG_HD bool pb_code_match(uint32_t x, uint32_t y)
{
	const uint32_t mx = x & 15, my = y & 15, lx = x >> 4, ly = y >> 4;
	return ((my & ~mx) == 0 && (lx | (ly ^ 1))) || ((mx & ~my) == 0 && (ly | (lx ^ 1)));
}

// One cell from its three neighbours (fd diagonal, fu / gu above, fl / hl left) and the score of its characters
ABG_HD uint32_t pb_cell(int fd, int fu, int gu, int fl, int hl, int s, int& f, int& g, int& h)
{
	const int go = fu + PB_GAP_OPEN, ge = gu + PB_GAP_EXTEND, ho = fl + PB_GAP_OPEN, he = hl + PB_GAP_EXTEND, d = fd + s;
	g = go > ge ? go : ge;
	h = ho > he ? ho : he;
	const int gh = g > h ? g : h;
	f = d > gh ? d : gh;
	return (f == d ? PB_DIAG : 0) | (f == g ? PB_VERT : 0) | (f == h ? PB_HORZ : 0) | (g == ge ? PB_VEXT : 0) | (h == he ? PB_HEXT : 0);
}

// backtrack from the flags.  The consensus is written backwards from cons_end (one past its last byte) where cons_end is not null;
// it starts at cons_end - size.  PB_VEXT is never set in row 1 nor PB_HEXT in column 1 (the cell above or left is INT_MIN / 2), which
// is the reference's assert(i > 0); the `> 1` below only keeps a walk over foreign bytes inside the pair.
ABG_HD void pb_traceback(const uint8_t* flags, uint64_t stride, const uint8_t* a, uint32_t la, const uint8_t* b, uint32_t lb, uint8_t* cons_end,
    uint32_t& matches, uint32_t& size)
{
	uint32_t i = la, j = lb, m = 0, n = 0;
	while (i > 0 && j > 0) {
		const uint32_t fl = flags[(uint64_t)(i - 1) * stride + (j - 1)];
		if (fl & PB_DIAG) {
			uint8_t c;
			if (pb_score(a[i - 1], b[j - 1], c) == PB_MATCH) m++;
			++n;
			if (cons_end) *(cons_end - n) = c;
			i--;
			j--;
		} else if (fl & PB_VERT) {
			while (i > 1 && (flags[(uint64_t)(i - 1) * stride + (j - 1)] & PB_VEXT)) {
				++n;
				if (cons_end) *(cons_end - n) = mc_tolower(a[i - 1]);
				i--;
			}
			++n;
			if (cons_end) *(cons_end - n) = mc_tolower(a[i - 1]);
			i--;
		} else { // PB_HORZ: f is one of the three
			while (j > 1 && (flags[(uint64_t)(i - 1) * stride + (j - 1)] & PB_HEXT)) {
				++n;
				if (cons_end) *(cons_end - n) = mc_tolower(b[j - 1]);
				j--;
			}
			++n;
			if (cons_end) *(cons_end - n) = mc_tolower(b[j - 1]);
			j--;
		}
	}
	for (; i > 0; i--) { ++n; if (cons_end) *(cons_end - n) = mc_tolower(a[i - 1]); }
	for (; j > 0; j--) { ++n; if (cons_end) *(cons_end - n) = mc_tolower(b[j - 1]); }
	matches = m;
	size = n;
}

// ---- host only from here

// alignGlobal, serially: the cells in the reference's order with two rolling rows, then the traceback.  cons may be null.
inline void pb_align_host(const uint8_t* a, uint32_t la, const uint8_t* b, uint32_t lb, uint32_t& matches, uint32_t& size, std::string* cons)
{
	const uint64_t stride = pb_stride(lb);
	std::vector<uint8_t> flags((size_t)(la * stride));
	std::vector<int> f(lb + 1), g(lb + 1);
	for (uint32_t j = 0; j <= lb; j++) { f[j] = pb_edge(j); g[j] = PB_NEG; }
	for (uint32_t i = 1; i <= la; i++) {
		int fd = f[0], fl = pb_edge(i), hl = PB_NEG;
		f[0] = fl;
		for (uint32_t j = 1; j <= lb; j++) {
			uint8_t c;
			int nf, ng, nh;
			flags[(size_t)((i - 1) * stride + (j - 1))] = (uint8_t)pb_cell(fd, f[j], g[j], fl, hl, pb_score(a[i - 1], b[j - 1], c), nf, ng, nh);
			fd = f[j];
			f[j] = fl = nf;
			g[j] = ng;
			hl = nh;
		}
	}
	std::vector<uint8_t> out(cons ? (size_t)la + lb : 0);
	pb_traceback(flags.data(), stride, a, la, b, lb, cons ? out.data() + out.size() : nullptr, matches, size);
	if (cons) cons->assign((const char*)out.data() + out.size() - size, size);
}

// alignMulti (alignGlobal.h:58-69) for three branches and more, alignPair for two: the consensus so far against the next branch.
// matches is min(0, ...) over the rounds, the reference's arithmetic, so it is 0 for a chain.
inline void pb_align_group_host(const std::vector<std::string>& seqs, uint32_t& matches, uint32_t& size, std::string* cons)
{
	std::string cur = seqs[0], next;
	uint32_t m = 0, n = (uint32_t)cur.size(), acc = 0;
	for (size_t j = 0; j + 1 < seqs.size(); j++) {
		pb_align_host((const uint8_t*)cur.data(), (uint32_t)cur.size(), (const uint8_t*)seqs[j + 1].data(), (uint32_t)seqs[j + 1].size(), m, n, &next);
		acc = acc < m ? acc : m;
		cur.swap(next);
	}
	matches = seqs.size() == 2 ? m : acc;
	size = n;
	if (cons) *cons = cur;
}

} // namespace abg
