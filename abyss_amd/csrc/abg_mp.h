// abg_mp.h -- the overlap alignment of abyss-mergepairs: which overlaps of read 1 with the reverse complement of read 2 it keeps.
//
// Reference behaviour restated here (ABySS 2.3.10, paths relative to the repo):
//   Align/mergepairs.cc:274-277        match 1, mismatch -2, gap_open = gap_extend = -10000
//   Align/smith_waterman.cpp:65-93     isMatch (abg_mc.h's mc_detail::is_match), matchScore, gapScore
//   Align/smith_waterman.cpp:195-241   the cell: the best of diagonal, up, left, the first on a tie; column 0 valid with score 0,
//                                      row 0 invalid from column 1 on
//   Align/smith_waterman.cpp:96-168    Backtrack from (N_a, j): along the parents until the parent lies on row 0 or column 0; that
//                                      last cell counts as a match or mismatch of its characters; 0 when it is past column 1 or
//                                      nothing matched
//   Align/smith_waterman.cpp:243-280   the last row's columns by score, std::sort, descending; stop at a score of exactly 0; after
//                                      the first success break if the next score is lower, and never again
//   Align/mergepairs.cc:162-205        matches >= m, then !(matches / length < identity), then isGapless
//
// No matrix is kept.  The parents form a tree, so what a backtrack returns is carried forwards: a cell whose parent is on the border
// starts (matches = isMatch, length = 1, start = i - 1, fail = j > 1), any other inherits its parent's, with length + 1 and, on a
// diagonal move, matches + isMatch.  All scores are integers; with both reads under MP_MAX_READ they fit an int, MP_NEG standing
// for the invalid row 0.
//
// Which overlaps are kept (mp_select), with R the columns before the first exact 0 in sorted order (every column when there is
// none), S the best score of a successful column of R, and G the columns of score S: one success in G, no failure beside it and a
// lower score somewhere is the early break, that one alone; one success, a failure beside it and a lower score somewhere depends on
// where std::sort put the two (MP_ORDER_DEPENDENT: mp_replay sorts the row as the reference does and walks it); anything else keeps
// every success of R.
//
// mp_cell, mp_select and mp_filter are the text the host and the kernel (abg_mp.hip) compile.
#pragma once
#include "abg_mc.h"

#include <algorithm>
#include <climits>
#include <cstdint>
#include <string>
#include <vector>

namespace abg {

constexpr int MP_MATCH = 1, MP_MISMATCH = -2, MP_GAP = -10000, MP_NEG = INT_MIN / 2;
constexpr uint32_t MP_MAX_READ = 100000;  // a read longer than this is refused: 2 * 100,000 * 10,000 is the last sum an int holds
constexpr uint32_t MP_KERNEL_MAX = 512;   // the longest read the kernel takes (abg_mp.hip says why)
constexpr uint32_t MP_FAIL = 0x80000000u; // in MPCell::start: the backtrack ends past column 1

enum { MP_ORDER_DEPENDENT = 1, MP_TOO_LONG = 2, MP_BREAK_TAKEN = 4, MP_BREAK_NOT_TAKEN = 8, MP_UNSPILLED = 16 };

// what a backtrack from this cell returns, and its score
struct MPCell { int32_t h; uint32_t matches, length, start; };

// a pair's answer (abg_mp_record of include/abyss_amd.h): the list's size after the alignment and after each filter; the overlap
// that is left when n_gapless is 1; the flags; where the kernel put the last row of an order-dependent pair (MPCells of the spill)
struct MPRecord { uint32_t n_aligned, n_matches, n_identity, n_gapless, t_pos, h_pos, length, matches, flags, spill; };

// a pair as the kernel takes it: read 1 at a_off and read 2 (as in the file: the kernel complements it) at b_off of the input
struct MPPair { uint64_t a_off, b_off; uint32_t la, lb; };

// bit (a, b) of the 256 x 256 table the host fills from is_match
ABG_HD bool mp_table_match(const uint32_t* table, uint8_t a, uint8_t b) { return (table[(uint32_t)a * 8 + (b >> 5)] >> (b & 31)) & 1; }

// Cell (i, j) from its diagonal, upper and left neighbours; move: where it is not null, the neighbour chosen (0, 1, 2 in that order)
ABG_HD MPCell mp_cell(const MPCell& d, const MPCell& u, const MPCell& l, bool match, uint32_t i, uint32_t j, uint8_t* move = nullptr)
{
	const int cd = d.h == MP_NEG ? MP_NEG : d.h + (match ? MP_MATCH : MP_MISMATCH), cu = u.h == MP_NEG ? MP_NEG : u.h + MP_GAP,
	          cl = l.h == MP_NEG ? MP_NEG : l.h + MP_GAP;
	int best = cd, which = 0;
	if (cu > best) { best = cu; which = 1; }
	if (cl > best) { best = cl; which = 2; }
	if (move) *move = (uint8_t)which;
	const bool border = which == 0 ? (i == 1 || j == 1) : which == 1 ? i == 1 : j == 1;
	MPCell c;
	c.h = best;
	if (border) {
		c.matches = match ? 1 : 0;
		c.length = 1;
		c.start = (i - 1) | (j > 1 ? MP_FAIL : 0);
	} else {
		const MPCell& p = which == 0 ? d : which == 1 ? u : l;
		c.matches = p.matches + (which == 0 && match ? 1 : 0);
		c.length = p.length + 1;
		c.start = p.start;
	}
	return c;
}

// the borders: column 0 of any row, and row 0 from column 1 on
ABG_HD MPCell mp_column0() { return MPCell{ 0, 0, 0, 0 }; }
ABG_HD MPCell mp_row0() { return MPCell{ MP_NEG, 0, 0, 0 }; }

ABG_HD bool mp_success(const MPCell& c) { return !(c.start & MP_FAIL) && c.matches > 0; }

// One kept overlap, ending at column j of the last row, through the three filters.  min_identity[L]: the smallest number of matches
// at which (double)matches / L < (double)identity is false, worked out by the host with that expression.
ABG_HD void mp_filter(MPRecord& r, const MPCell& c, uint32_t j, uint32_t la, uint32_t min_matches, const uint32_t* min_identity)
{
	r.n_aligned++;
	if (c.matches < min_matches) return;
	r.n_matches++;
	if (c.matches < min_identity[c.length]) return;
	r.n_identity++;
	if (!(c.length == la - c.start && c.length == j)) return; // isGapless: length == |a| - t_pos && length == h_pos + 1
	if (++r.n_gapless == 1) { r.t_pos = c.start; r.h_pos = j - 1; r.length = c.length; r.matches = c.matches; }
}

// How mp_select's loops are shared out: the host has one lane; the kernel's 64 lanes take every 64th column and reduce over the wave
struct MPSerial {
	ABG_HD uint32_t first() const { return 0; }
	ABG_HD uint32_t step() const { return 1; }
	ABG_HD bool any(bool x) const { return x; }
	ABG_HD int max(int x) const { return x; }
	ABG_HD uint32_t sum(uint32_t x) const { return x; }
};

// From the last row (row[j - 1]: column j; any type with such an operator[]): the record, or MP_ORDER_DEPENDENT and nothing else.
// The overlap's four fields are set when exactly one is left, and 0 otherwise.
template <class Row, class Par>
ABG_HD void mp_select(const Row& row, uint32_t la, uint32_t lb, uint32_t min_matches, const uint32_t* min_identity, MPRecord& r, const Par& par)
{
	r = MPRecord{ 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 };
	if (la == 0 || lb == 0) return; // (row 0 is all zeros in the reference: the loop stops at its first column)
	bool zero = false;
	for (uint32_t j = par.first(); j < lb; j += par.step()) zero = zero || row[j].h == 0;
	const bool has_zero = par.any(zero);
	int mine = INT_MIN;
	for (uint32_t j = par.first(); j < lb; j += par.step()) {
		const MPCell c = row[j];
		if ((!has_zero || c.h > 0) && mp_success(c) && c.h > mine) mine = c.h;
	}
	const int best = par.max(mine);
	if (best == INT_MIN) return;
	uint32_t wins = 0, fails = 0, only = 0;
	bool lower = false;
	for (uint32_t j = par.first(); j < lb; j += par.step()) {
		const MPCell c = row[j];
		if (c.h == best) {
			if (mp_success(c)) { wins++; only += j; } else fails++;
		} else if (c.h < best)
			lower = true;
	}
	wins = par.sum(wins);
	fails = par.sum(fails);
	only = par.sum(only); // (the column itself when wins is 1)
	lower = par.any(lower);
	if (wins == 1 && fails > 0 && lower) { r.flags = MP_ORDER_DEPENDENT; return; }
	MPRecord part = r;
	if (wins == 1) { // alone in its group: the break after it, or nothing below it to go on to
		if (par.first() == 0) mp_filter(part, row[only], only + 1, la, min_matches, min_identity);
	} else {
		for (uint32_t j = par.first(); j < lb; j += par.step()) {
			const MPCell c = row[j];
			if ((!has_zero || c.h > 0) && mp_success(c)) mp_filter(part, c, j + 1, la, min_matches, min_identity);
		}
	}
	r.n_aligned = par.sum(part.n_aligned);
	r.n_matches = par.sum(part.n_matches);
	r.n_identity = par.sum(part.n_identity);
	r.n_gapless = par.sum(part.n_gapless);
	const bool one = r.n_gapless == 1; // then one lane holds it, and only that lane's fields are set
	r.t_pos = par.sum(one ? part.t_pos : 0);
	r.h_pos = par.sum(one ? part.h_pos : 0);
	r.length = par.sum(one ? part.length : 0);
	r.matches = par.sum(one ? part.matches : 0);
	r.flags = wins == 1 && lower ? MP_BREAK_TAKEN : MP_BREAK_NOT_TAKEN;
}

// ---- host only from here

// min_identity[0 .. max_length]
inline std::vector<uint32_t> mp_identity_table(float identity, uint32_t max_length)
{
	std::vector<uint32_t> t(max_length + 1, 0);
	for (uint32_t L = 1; L <= max_length; L++) {
		uint32_t lo = 0, hi = L + 1; // the test is monotone in the matches; L + 1 stands for "never"
		auto low = [&](uint32_t m) { return (double)m / L < identity; };
		if (!low(0)) { t[L] = 0; continue; }
		if (low(L)) { t[L] = L + 1; continue; }
		lo = 0, hi = L; // low(lo), !low(hi)
		while (hi - lo > 1) { const uint32_t mid = lo + (hi - lo) / 2; if (low(mid)) lo = mid; else hi = mid; }
		t[L] = hi;
	}
	return t;
}

inline std::vector<uint32_t> mp_match_table()
{
	std::vector<uint32_t> t(256 * 8, 0);
	for (int a = 0; a < 256; a++)
		for (int b = 0; b < 256; b++) {
			char c;
			if (mc_detail::is_match((char)a, (char)b, c)) t[a * 8 + (b >> 5)] |= 1u << (b & 31);
		}
	return t;
}

inline std::string mp_reverse_complement(const std::string& s)
{
	std::string rc(s.rbegin(), s.rend());
	for (char& c : rc) c = (char)ov_complement((uint8_t)c);
	return rc;
}

// Where the reference's isMatch would reach ambiguityToBitmask with a byte that is no code and assert: a cell whose diagonal is
// valid (every cell but those of row 1 past column 1), the two characters unequal in either case and neither an N.
inline bool mp_pair_asserts(const std::string& a, const std::string& b)
{
	if (a.empty() || b.empty()) return false;
	size_t in_a[256] = { 0 }, in_b[256] = { 0 };
	for (unsigned char c : a) in_a[c]++;
	for (unsigned char c : b) in_b[c]++;
	auto other_case = [](unsigned char c) { return mc_lower(c) ? mc_upper(c) : mc_tolower(c); };
	auto passes = [&](unsigned char c, const size_t* in, unsigned char first) { // how many of the reachable characters need no mask
		// (reachable: all of the other read, or its first character alone)
		if (first) return (size_t)(first == c || first == other_case(c) || first == 'N' || first == 'n');
		return in[c] + (other_case(c) != c ? in[other_case(c)] : 0) + in[(unsigned char)'N'] + in[(unsigned char)'n'];
	};
	for (size_t i = 0; i < a.size(); i++)
		if (!mc_mask(mc_upper((uint8_t)a[i]))) {
			if (i == 0 ? !passes((unsigned char)a[i], in_b, (unsigned char)b[0]) : passes((unsigned char)a[i], in_b, 0) < b.size()) return true;
		}
	for (size_t j = 0; j < b.size(); j++)
		if (!mc_mask(mc_upper((uint8_t)b[j]))) {
			if (j == 0) { if (passes((unsigned char)b[j], in_a, 0) < a.size()) return true; }
			else if (a.size() > 1 && passes((unsigned char)b[j], in_a, 0) - passes((unsigned char)b[j], in_a, (unsigned char)a[0]) < a.size() - 1) return true;
		}
	return false;
}

// The last row of the dynamic programme of a against b (b already reverse-complemented), two rolling rows.  which: where it is not
// null, la * lb bytes, the move each cell chose (0 diagonal, 1 up, 2 left), for the print of -vvv.
inline void mp_last_row_host(const std::string& a, const std::string& b, std::vector<MPCell>& row, std::vector<uint8_t>* which = nullptr)
{
	const uint32_t la = (uint32_t)a.size(), lb = (uint32_t)b.size();
	row.assign(lb, mp_row0());
	if (which) which->assign((size_t)la * lb, 0);
	for (uint32_t i = 1; i <= la; i++) {
		MPCell diag = mp_column0(), left = mp_column0();
		for (uint32_t j = 1; j <= lb; j++) {
			char c;
			const MPCell up = row[j - 1];
			const MPCell cell = mp_cell(diag, up, left, mc_detail::is_match(a[i - 1], b[j - 1], c), i, j, which ? &(*which)[(size_t)(i - 1) * lb + (j - 1)] : nullptr);
			diag = up;
			row[j - 1] = left = cell;
		}
	}
}

struct MPIndexCmp { // index_cmp<double*>, smith_waterman.cpp:55-60
	const double* arr;
	bool operator()(const int a, const int b) const { return arr[a] > arr[b]; }
};

// The reference's own loop over the last row, sorted by the same std::sort call on the same doubles: the record, and the column of
// the first success (0: none), whose alignment -vvv prints.
inline uint32_t mp_replay(const MPCell* row, uint32_t la, uint32_t lb, uint32_t min_matches, const uint32_t* min_identity, MPRecord& r)
{
	r = MPRecord{ 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 };
	if (la == 0 || lb == 0) return 0;
	std::vector<double> H(lb + 1, 0.0);
	for (uint32_t j = 1; j <= lb; j++) H[j] = row[j - 1].h;
	std::vector<int> order(lb);
	for (uint32_t j = 0; j < lb; j++) order[j] = (int)j + 1;
	std::sort(order.data(), order.data() + lb, MPIndexCmp{ H.data() });
	uint32_t first = 0;
	for (uint32_t j = 0; j < lb; j++) {
		const int jmax = order[j];
		if (H[jmax] == 0) break;
		if (!mp_success(row[jmax - 1])) continue;
		mp_filter(r, row[jmax - 1], (uint32_t)jmax, la, min_matches, min_identity);
		if (!first) {
			first = (uint32_t)jmax;
			if (j + 1 < lb && H[order[j + 1]] < H[jmax]) { r.flags |= MP_BREAK_TAKEN; break; }
			r.flags |= MP_BREAK_NOT_TAKEN;
		}
	}
	if (r.n_gapless != 1) r.t_pos = r.h_pos = r.length = r.matches = 0;
	return first;
}

// alignOverlap and filterAlignments of one pair on the host: a is read 1, b the reverse complement of read 2
inline void mp_align_host(const std::string& a, const std::string& b, uint32_t min_matches, const uint32_t* min_identity, MPRecord& r)
{
	std::vector<MPCell> row;
	mp_last_row_host(a, b, row);
	mp_select(row.data(), (uint32_t)a.size(), (uint32_t)b.size(), min_matches, min_identity, r, MPSerial());
	if (r.flags & MP_ORDER_DEPENDENT) {
		mp_replay(row.data(), (uint32_t)a.size(), (uint32_t)b.size(), min_matches, min_identity, r);
		r.flags |= MP_ORDER_DEPENDENT;
	}
}

} // namespace abg
