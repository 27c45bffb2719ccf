// abg_mc.h -- the sequence merge of MergeContigs (bin/abyss-pe:600-892): the bytes of a path of contigs spliced at their overlaps.
//
// Reference behaviour restated here (ABySS 2.3.10, paths relative to the repo):
//   MergePaths/MergeContigs.cpp:159-171  sequence(node): the contig, its reverse complement, or k - 1 'N' and the gap's n 'N' (lowercase when n < k)
//   MergePaths/MergeContigs.cpp:176-197  createConsensus: equal characters, N gives way, a subset code joins, case is kept as a mask
//   MergePaths/MergeContigs.cpp:213-277  mergeContigs: consensus of the tail of the sequence so far and the head of the next node, the
//                                        chomp(seq, 'n') retry, the overlap alignment, the warning block
//   Common/Sequence.cpp:141-204, Sequence.h:94-115   the ambiguity codes as bit masks, and / or / subset
//   Align/smith_waterman.cpp:33-292      alignOverlap: the alignment pinned at the end of a and the start of b, its print
//
// The store: the contigs' bytes end to end, case and IUPAC codes as the file has them (FastaReader::NO_FOLD_CASE), MC_PAD zero
// bytes before and after.  A node is 2 * contig + sense, or -n for the gap of n.  Character p of a node is one byte of the store, the
// complement (abg_ov.h's table) of one, or an N: mc_node_char.
//
// The device runs the common case in two kernels (abg_mc.hip): mc_junction walks the junctions of a path in order, a wave a path,
// lanes over the overlap window, with the last MC_RING characters of the sequence so far in LDS, because the window after a
// junction is the tail of `consensus + s[ov:]`, not of the contig: a contig shorter than the two overlaps around it shows the next
// junction the consensus of the one before.  It writes every junction's consensus to a side buffer and flags the path whose
// junction has none.  mc_splice then writes the output bytes flat, in tiles, from a list of segments (consensus slice, contig
// forwards, contig backwards complemented, gap run) laid out by mc_layout below.  A flagged path is merged on the host by
// mc_merge_path_host, the whole of mergeContigs with its retry and alignment: rare, and the same text for host and checker.
#pragma once
#include "abg_ov.h"

#include <algorithm>
#include <cfloat>
#include <cstdio>
#include <string>
#include <vector>

namespace abg {

constexpr uint32_t MC_RING = 1024;  // characters of tail a wave keeps; a path with a larger overlap is merged on the host
constexpr uint64_t MC_PAD = 32;     // zero bytes around the store: the splice builds 16 bytes from three aligned words, forwards and backwards
constexpr int MC_BLOCK = 256;       // threads of a splice tile

enum { MC_SEG_CONSENSUS = 0, MC_SEG_FORWARD = 1, MC_SEG_REVERSE = 2, MC_SEG_GAP = 3 };

// Output bytes start .. (the next segment's start) of the flat output.  src: for CONSENSUS an offset of the side buffer, for FORWARD
// the store offset of the first byte, for REVERSE the store offset of the byte complemented first (the bytes before it follow), for
// GAP the character of the run.
struct MCSeg { uint64_t start, src; uint32_t kind, path; };

struct MCStore { const uint8_t* bytes; const uint64_t* off; uint64_t n; }; // bytes[off[i] .. off[i + 1]): contig i

ABG_HD bool mc_lower(uint8_t c) { return c >= 'a' && c <= 'z'; }
ABG_HD uint8_t mc_upper(uint8_t c) { return mc_lower(c) ? (uint8_t)(c - 32) : c; }
ABG_HD uint8_t mc_tolower(uint8_t c) { return c >= 'A' && c <= 'Z' ? (uint8_t)(c + 32) : c; }
ABG_HD bool mc_acgt(uint8_t c) { const uint8_t u = mc_upper(c); return u == 'A' || u == 'C' || u == 'G' || u == 'T'; }

// ambiguityToBitmask (Sequence.cpp:141-179) of an uppercase letter; 0 where the reference asserts
ABG_HD unsigned mc_mask(uint8_t u)
{
	switch (u) {
	case 'A': return 0x1; case 'B': return 0xe; case 'C': return 0x2; case 'D': return 0xd; case 'G': return 0x4; case 'H': return 0xb;
	case 'K': return 0xc; case 'M': return 0x3; case 'N': return 0xf; case 'R': return 0x5; case 'S': return 0x6; case 'T': return 0x8;
	case 'V': return 0x7; case 'W': return 0x9; case 'Y': return 0xa;
	default: return 0;
	}
}
// bitmaskToAmbiguity (Sequence.cpp:182-204)
ABG_HD uint8_t mc_unmask(unsigned x)
{
	const uint64_t lo = 0x565352474d43414eull, hi = 0x4e42444b48595754ull; // "NACMGRSV", "TWYHKDBN", lowest byte first
	return (uint8_t)((x < 8 ? lo >> (8 * x) : hi >> (8 * (x - 8))) & 0xff);
}

// One character of createConsensus (MergeContigs.cpp:184-195); 0 where it gives up
ABG_HD uint8_t mc_consensus_char(uint8_t a, uint8_t b)
{
	const bool mask = mc_lower(a) || mc_lower(b);
	const uint8_t ca = mc_upper(a), cb = mc_upper(b);
	uint8_t c;
	if (ca == cb) c = ca;
	else if (ca == 'N') c = cb;
	else if (cb == 'N') c = ca;
	else {
		const unsigned ma = mc_mask(ca), mb = mc_mask(cb), both = ma & mb;
		if (ma == 0 || mb == 0 || (both != ma && both != mb)) return 0; // (no code has mask 0; the reference asserts on such a byte)
		c = mc_unmask(ma | mb);
	}
	return mask ? mc_tolower(c) : c;
}

ABG_HD uint64_t mc_node_len(const MCStore& st, int32_t node, uint32_t k)
{
	return node < 0 ? (uint64_t)(k - 1) + (uint64_t)(-(int64_t)node) : st.off[((uint32_t)node >> 1) + 1] - st.off[(uint32_t)node >> 1];
}
ABG_HD uint8_t mc_gap_char(int32_t node, uint32_t k, uint64_t p) { return p >= k - 1 && (uint64_t)(-(int64_t)node) < k ? 'n' : 'N'; }
ABG_HD uint8_t mc_node_char(const MCStore& st, int32_t node, uint32_t k, uint64_t p)
{
	if (node < 0) return mc_gap_char(node, k, p);
	const uint32_t id = (uint32_t)node >> 1;
	return (node & 1) ? ov_complement(st.bytes[st.off[id + 1] - 1 - p]) : st.bytes[st.off[id] + p];
}

// ---- host only from here

// The segments of one path whose every junction has a consensus, appended to segs with output positions from `at`; the path's
// length is returned.  A junction's window is the tail of what is laid so far, so it cuts the segments laid before it from the
// back.  false: an overlap longer than the node or than the sequence so far (the reference asserts).
inline bool mc_layout(const MCStore& st, uint32_t k, const int32_t* nodes, const uint32_t* ov, uint64_t n, uint32_t path, uint64_t at, uint64_t side,
    std::vector<MCSeg>& segs, uint64_t* length)
{
	const size_t first = segs.size();
	uint64_t end = at;
	auto slice = [&](int32_t node, uint64_t from, uint64_t to) { // characters from .. to of the node, at `end`
		if (from >= to) return;
		if (node < 0) {
			const uint8_t head = 'N', tail = mc_gap_char(node, k, k - 1);
			if (from < k - 1) { segs.push_back(MCSeg{ end, head, MC_SEG_GAP, path }); if (tail == head || to <= k - 1) { end += to - from; return; } end += k - 1 - from; from = k - 1; }
			segs.push_back(MCSeg{ end, tail, MC_SEG_GAP, path });
			end += to - from;
			return;
		}
		const uint32_t id = (uint32_t)node >> 1;
		if (node & 1) segs.push_back(MCSeg{ end, st.off[id + 1] - 1 - from, MC_SEG_REVERSE, path });
		else segs.push_back(MCSeg{ end, st.off[id] + from, MC_SEG_FORWARD, path });
		end += to - from;
	};
	for (uint64_t j = 0; j < n; ++j) {
		const uint64_t len = mc_node_len(st, nodes[j], k);
		if (j == 0) { slice(nodes[0], 0, len); continue; }
		const uint64_t o = ov[j];
		if (o > len || o > end - at) return false;
		const uint64_t a = end - o;
		while (segs.size() > first && segs.back().start >= a) segs.pop_back();
		segs.push_back(MCSeg{ a, side, MC_SEG_CONSENSUS, path });
		side += o;
		end = a + o;
		slice(nodes[j], o, len);
	}
	*length = end - at;
	return true;
}

namespace mc_detail {

// isMatch, smith_waterman.cpp:65-80, with ambiguityOr / ambiguityIsSubset on characters of either case (Sequence.h:94-115)
ABG_HD char ambiguity(char a, char b, bool isor) // (host and device: abg_pb.h scores with it too)
{
	const unsigned ma = mc_mask(mc_upper((uint8_t)a)), mb = mc_mask(mc_upper((uint8_t)b));
	const char c = (char)mc_unmask(isor ? (ma | mb) : (ma & mb));
	const bool la = mc_lower((uint8_t)a), lb = mc_lower((uint8_t)b);
	return (isor ? (la || lb) : (la && lb)) ? (char)mc_tolower((uint8_t)c) : c;
}
inline bool is_match(char a, char b, char& c)
{
	if (a == b) c = a;
	else if (mc_upper((uint8_t)a) == mc_upper((uint8_t)b)) c = mc_lower((uint8_t)a) || mc_lower((uint8_t)b) ? (char)mc_tolower((uint8_t)a) : a;
	else if (a == 'N' || a == 'n') c = b;
	else if (b == 'N' || b == 'n') c = a;
	else {
		c = ambiguity(a, b, true);
		const char both = ambiguity(a, b, false);
		return both == a || both == b;
	}
	return true;
}

struct Overlap { unsigned t_pos = 0, h_pos = 0, matches = 0; std::string str; };

// alignOverlap(a, b, 0, overlaps, false, verbose), smith_waterman.cpp:96-292: the first alignment that backtracks to the first
// column, highest score of the last row first, as std::sort orders the row under the reference's comparator
inline bool align_overlap(const std::string& a, const std::string& b, bool verbose, Overlap& out, std::string& log)
{
	const int na = (int)a.size(), nb = (int)b.size(), w = nb + 1;
	std::vector<double> H((size_t)(na + 1) * w, 0.0);
	std::vector<int> Ii((size_t)(na + 1) * w, 0), Ij((size_t)(na + 1) * w, 0);
	std::vector<char> V((size_t)(na + 1) * w, 0);
	auto at = [w](int i, int j) { return (size_t)i * w + j; };
	for (int i = 0; i <= na; i++) { Ii[at(i, 0)] = i - 1; V[at(i, 0)] = 1; }
	for (int j = 0; j <= nb; j++) { Ij[at(0, j)] = j - 1; V[at(0, j)] = 0; }
	V[at(0, 0)] = 1;
	for (int i = 1; i <= na; i++)
		for (int j = 1; j <= nb; j++) {
			char c;
			const double scores[3] = { V[at(i - 1, j - 1)] ? H[at(i - 1, j - 1)] + (is_match(a[i - 1], b[j - 1], c) ? 5 : -4) : -DBL_MAX,
				V[at(i - 1, j)] ? H[at(i - 1, j)] + (Ij[at(i - 1, j)] == j ? -4 : -12) : -DBL_MAX,
				V[at(i, j - 1)] ? H[at(i, j - 1)] + (Ii[at(i, j - 1)] == i ? -4 : -12) : -DBL_MAX };
			const int best = (int)(std::max_element(scores, scores + 3) - scores);
			H[at(i, j)] = scores[best];
			Ii[at(i, j)] = best == 2 ? i : i - 1;
			Ij[at(i, j)] = best == 1 ? j : j - 1;
			V[at(i, j)] = H[at(i, j)] == -DBL_MAX ? 0 : 1;
		}
	std::vector<int> order(nb);
	for (int j = 0; j < nb; j++) order[j] = j + 1;
	const double* last = &H[at(na, 0)];
	std::sort(order.begin(), order.end(), [last](const int x, const int y) { return last[x] > last[y]; });
	for (int jj = 0; jj < nb; jj++) {
		const int jmax = order[jj];
		if (last[jmax] == 0) break;
		// Backtrack, smith_waterman.cpp:96-168
		int ci = na, cj = jmax, ni = Ii[at(ci, cj)], nj = Ij[at(ci, cj)];
		std::string qa, ta, match;
		unsigned matches = 0;
		auto pair = [&](int i, int j) {
			char c;
			if (is_match(a[i - 1], b[j - 1], c)) { match += c; matches++; }
			else match += ambiguity(a[i - 1], b[j - 1], true);
		};
		while ((ci != ni || cj != nj) && nj != 0 && ni != 0) {
			if (ni == ci) { qa += '-'; match += (char)tolower((unsigned char)b[cj - 1]); ta += b[cj - 1]; }
			else {
				qa += a[ci - 1];
				if (nj == cj) { ta += '-'; match += (char)tolower((unsigned char)a[ci - 1]); }
				else { ta += b[cj - 1]; pair(ci, cj); }
			}
			ci = ni; cj = nj;
			ni = Ii[at(ci, cj)]; nj = Ij[at(ci, cj)];
		}
		if (cj > 1) continue;
		qa += a[ci - 1];
		ta += b[cj - 1];
		pair(ci, cj);
		if (matches == 0) continue;
		std::reverse(qa.begin(), qa.end());
		std::reverse(ta.begin(), ta.end());
		std::reverse(match.begin(), match.end());
		out.t_pos = (unsigned)(ci - 1);
		out.h_pos = (unsigned)(jmax - 1);
		out.matches = matches;
		out.str = match;
		if (verbose) { // printAlignment, smith_waterman.cpp:33-52
			const unsigned astart = out.t_pos;
			log += a.substr(0, astart) + qa + '\n' + std::string(astart, ' ');
			for (size_t i = 0; i < match.size(); i++) log += (match[i] == qa[i] || match[i] == ta[i]) ? '.' : match[i];
			log += '\n' + std::string(astart, ' ') + ta + b.substr(out.h_pos + 1) + '\n';
		}
		return true;
	}
	return false;
}

} // namespace mc_detail

// In a log, \x01 <j> \x02 stands for the name of node j of the path and \x03 for the path as the reference prints it: the caller,
// who knows the names, puts them in.
//
// mergePath's sequence (MergeContigs.cpp:295-308) with the whole of mergeContigs.  seq: the merged sequence; log: what the
// reference writes to stderr on the way.  false with err set where the reference asserts.
inline bool mc_merge_path_host(const MCStore& st, uint32_t k, const int32_t* nodes, const uint32_t* ov, uint64_t n, int verbose, std::string& seq,
    std::string& log, std::string& err)
{
	auto sequence = [&](int32_t node) {
		std::string s((size_t)mc_node_len(st, node, k), 'N');
		for (size_t p = 0; p < s.size(); ++p) s[p] = (char)mc_node_char(st, node, k, p);
		return s;
	};
	seq.clear();
	for (uint64_t j = 0; j < n; ++j) {
		if (seq.empty()) { seq = sequence(nodes[j]); continue; }
		const size_t overlap = ov[j];
		const std::string s = sequence(nodes[j]);
		if (s.size() < overlap) { err = "node " + std::to_string(j) + " of a path is shorter than its overlap of " + std::to_string(overlap); return false; }
		const std::string bo(s, 0, overlap);
		std::string ao;
		bool done = false;
		do {
			if (seq.size() < overlap) { err = "the sequence before node " + std::to_string(j) + " of a path is shorter than its overlap of " + std::to_string(overlap); return false; }
			ao = seq.substr(seq.size() - overlap);
			std::string o(overlap, '\0');
			bool ok = true;
			for (size_t i = 0; i < overlap && ok; ++i) ok = (o[i] = (char)mc_consensus_char((uint8_t)ao[i], (uint8_t)bo[i])) != 0;
			if (ok) {
				seq.resize(seq.size() - overlap);
				seq += o;
				seq.append(s, overlap, std::string::npos);
				done = true;
				break;
			}
		} while (!seq.empty() && seq.back() == 'n' && (seq.pop_back(), true)); // chomp(seq, 'n')
		if (done) continue;
		if (verbose > 2) log += '\n';
		mc_detail::Overlap o;
		bool good = false;
		if (mc_detail::align_overlap(ao, bo, verbose > 2, o, log)) {
			const float identity = (float)o.matches / o.str.size();
			good = o.matches >= 20 && identity >= 0.9f;
			if (verbose > 2) {
				char buf[96];
				snprintf(buf, sizeof buf, "%u / %zu = %g%s\n", o.matches, o.str.size(), (double)identity,
				    o.matches < 20 ? " (too few)" : identity < 0.9f ? " (too low)" : " (good)");
				log += buf;
			}
		}
		if (good) {
			seq.erase(seq.size() - overlap + o.t_pos);
			seq += o.str;
			seq.append(s, o.h_pos + 1, std::string::npos);
		} else {
			log += "warning: the head of \x01" + std::to_string(j) + "\x02 does not match the tail of the previous contig\n" + ao + '\n' + bo + "\n\x03\n";
			seq += 'n';
			seq += s;
		}
	}
	return true;
}

} // namespace abg
