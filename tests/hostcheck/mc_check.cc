// mc_check -- MergeContigs without a GPU, for the CPU suite: the same mergecontigs_core.h as abyss_amd/bin/MergeContigs over the
// serial text of abg_mc.h (what the kernels must equal, and what the product runs for the paths they flag).
//   mc_check run ARGS...        what `MergeContigs ARGS...` writes (the -o and -g files, stdout, stderr, status)
//   mc_check splice FILE        the paths of a dump (tests/mergecontigs_golden.py dump_paths) merged the way the device merges them: the
//                               junction walk over a ring, then the output bytes from mc_layout's segments alone.  A line a path:
//                               sequence, flag (0; 1 a junction without consensus, 2 a window the ring cannot hold: merged by
//                               mc_merge_path_host), ACGT count; then "# segments" with the number of each kind and of two-part gaps.
//                               Status 1 for an empty segment or one that starts before its predecessor.
#include "../../abyss_amd/csrc/abg_mc.h"
#include "../../abyss_amd/csrc/host/mergecontigs_core.h"

#include <fstream>

namespace {

struct SerialMerger : mc::Merger {
	std::vector<uint8_t> store;
	std::vector<uint64_t> off;
	std::string seqs_, logs_;
	bool open(std::string&) override { return true; }
	bool set_contigs(const std::string& bytes, const std::vector<uint64_t>& offsets, std::string&) override
	{
		store.assign(bytes.size() + 2 * abg::MC_PAD, 0);
		memcpy(store.data() + abg::MC_PAD, bytes.data(), bytes.size());
		off = offsets;
		return true;
	}
	bool merge(uint32_t k, const std::vector<uint64_t>& noff, const std::vector<mc::Node>& nodes, const std::vector<uint32_t>& ov, int verbose,
	    std::vector<uint64_t>& soff, const uint8_t*& seqs, std::vector<uint64_t>& acgt, std::vector<uint64_t>& loff, const char*& logs, std::string& err) override
	{
		const abg::MCStore st{ store.data() + abg::MC_PAD, off.data(), off.size() - 1 };
		seqs_.clear();
		logs_.clear();
		soff.assign(1, 0);
		loff.assign(1, 0);
		acgt.clear();
		std::string seq, log;
		for (size_t i = 0; i + 1 < noff.size(); ++i) {
			for (uint64_t j = noff[i]; j < noff[i + 1]; ++j)
				if (nodes[j] >= 0 && (nodes[j] & 1))
					for (uint64_t p = off[(size_t)nodes[j] >> 1]; p < off[((size_t)nodes[j] >> 1) + 1]; ++p)
						if (!abg::ov_complement(st.bytes[p])) { err = "path " + std::to_string(i) + ": contig " + std::to_string(nodes[j] >> 1) + " holds a character that has no complement"; return false; }
			log.clear();
			if (!abg::mc_merge_path_host(st, k, nodes.data() + noff[i], ov.data() + noff[i], noff[i + 1] - noff[i], verbose, seq, log, err)) {
				err = "path " + std::to_string(i) + ": " + err;
				return false;
			}
			seqs_ += seq;
			logs_ += log;
			soff.push_back(seqs_.size());
			loff.push_back(logs_.size());
			acgt.push_back((uint64_t)std::count_if(seq.begin(), seq.end(), [](char c) { return abg::mc_acgt((uint8_t)c); }));
		}
		seqs = (const uint8_t*)seqs_.data();
		logs = logs_.c_str();
		return true;
	}
};

// What abg_mc_merge does with one batch, without a device.  The layout is the product's own (mc_layout); the junction pass is
// mc_junction_kernel's text with the lanes of a window one after the other (a lane reads and writes its own ring slot only, a window
// being no longer than the ring); the output is then written from the segments and nothing else, as mc_splice_kernel writes it.
int splice(const char* file)
{
	std::ifstream in(file);
	uint32_t k = 0;
	uint64_t nc = 0, np = 0;
	if (!(in >> k >> nc >> np) || k == 0) { fprintf(stderr, "mc_check: %s: no dump of paths\n", file); return 2; }
	std::vector<uint8_t> store(abg::MC_PAD, 0);
	std::vector<uint64_t> off(1, 0), noff(1, 0);
	std::vector<int32_t> nodes;
	std::vector<uint32_t> ov;
	std::string word;
	for (uint64_t i = 0; i < nc && (in >> word); ++i) {
		store.insert(store.end(), word.begin(), word.end());
		off.push_back(store.size() - abg::MC_PAD);
	}
	store.resize(store.size() + abg::MC_PAD, 0);
	for (uint64_t i = 0; i < np; ++i) {
		uint64_t n = 0;
		in >> n;
		for (uint64_t j = 0; j < n; ++j) {
			int64_t u = 0;
			uint32_t o = 0;
			in >> u >> o;
			if (u >= 0 && (uint64_t)(u >> 1) >= nc) { fprintf(stderr, "mc_check: path %llu: no such contig\n", (unsigned long long)i); return 2; }
			nodes.push_back((int32_t)u);
			ov.push_back(o);
		}
		noff.push_back(nodes.size());
	}
	if (!in || off.size() != nc + 1) { fprintf(stderr, "mc_check: %s: the dump ends early\n", file); return 2; }
	const abg::MCStore st{ store.data() + abg::MC_PAD, off.data(), nc };

	struct Path { uint64_t at = 0, side = 0, length = 0; uint32_t window = 0; int flag = 0; }; // flag 2: the host's from the start
	std::vector<Path> paths(np);
	std::vector<abg::MCSeg> segs;
	uint64_t total = 0, side = 0;
	for (uint64_t i = 0; i < np; ++i) {
		Path& p = paths[i];
		const uint64_t first = noff[i], n = noff[i + 1] - first;
		for (uint64_t j = 1; j < n; ++j) p.window = std::max(p.window, ov[first + j]);
		p.at = total;
		p.side = side;
		const size_t mark = segs.size();
		if (p.window > abg::MC_RING || !abg::mc_layout(st, k, nodes.data() + first, ov.data() + first, n, (uint32_t)i, total, side, segs, &p.length)) {
			segs.resize(mark);
			p.length = 0;
			p.flag = 2;
			continue;
		}
		for (uint64_t j = 1; j < n; ++j) side += ov[first + j];
		total += p.length;
	}
	// no empty segment, none before its predecessor, each inside its own path
	uint64_t kinds[4] = { 0, 0, 0, 0 }, two_part = 0;
	for (size_t s = 0; s < segs.size(); ++s) {
		const abg::MCSeg& g = segs[s];
		const uint64_t next = s + 1 < segs.size() ? segs[s + 1].start : total;
		const bool heads = s == 0 || segs[s - 1].path != g.path;
		if (g.kind > abg::MC_SEG_GAP || g.path >= np || next <= g.start || (s == 0 && g.start != 0) || (heads && g.start != paths[g.path].at) ||
		    g.start >= paths[g.path].at + paths[g.path].length) {
			fprintf(stderr, "mc_check: segment %zu of path %u: bytes %llu .. %llu\n", s, g.path, (unsigned long long)g.start, (unsigned long long)next);
			return 1;
		}
		kinds[g.kind]++;
		if (!heads && g.kind == abg::MC_SEG_GAP && segs[s - 1].kind == abg::MC_SEG_GAP && segs[s - 1].src != g.src) two_part++;
	}

	std::vector<uint8_t> sidebuf(side, 0);
	for (uint64_t i = 0; i < np; ++i) {
		Path& p = paths[i];
		if (p.flag || noff[i + 1] - noff[i] < 2) continue;
		uint8_t ring[abg::MC_RING] = { 0 };
		const int32_t* nd = nodes.data() + noff[i];
		const uint32_t* o = ov.data() + noff[i];
		uint64_t end = abg::mc_node_len(st, nd[0], k), soff = p.side;
		const uint64_t cnt0 = std::min<uint64_t>(end, p.window);
		for (uint64_t q = 0; q < cnt0; ++q) {
			const uint64_t pos = end - cnt0 + q;
			ring[pos & (abg::MC_RING - 1)] = abg::mc_node_char(st, nd[0], k, pos);
		}
		for (uint64_t j = 1; j < noff[i + 1] - noff[i] && !p.flag; ++j) {
			const uint32_t w = o[j];
			const uint64_t len = abg::mc_node_len(st, nd[j], k);
			for (uint32_t q = 0; q < w; ++q) {
				const uint64_t pos = end - w + q;
				const uint8_t c = abg::mc_consensus_char(ring[pos & (abg::MC_RING - 1)], abg::mc_node_char(st, nd[j], k, q));
				if (c == 0) p.flag = 1;
				else { ring[pos & (abg::MC_RING - 1)] = c; sidebuf.at(soff + q) = c; }
			}
			soff += w;
			const uint64_t rest = len - w, cnt = std::min<uint64_t>(rest, p.window);
			for (uint64_t q = 0; q < cnt; ++q) {
				const uint64_t at = rest - cnt + q;
				ring[(end + at) & (abg::MC_RING - 1)] = abg::mc_node_char(st, nd[j], k, w + at);
			}
			end += rest;
		}
	}

	std::vector<uint8_t> out(total, 0);
	std::vector<uint64_t> counts(np, 0);
	for (size_t s = 0; s < segs.size(); ++s) {
		const abg::MCSeg& g = segs[s];
		const uint64_t next = s + 1 < segs.size() ? segs[s + 1].start : total;
		for (uint64_t pos = g.start; pos < next; ++pos) {
			const uint64_t d = pos - g.start;
			uint8_t ch;
			if (g.kind == abg::MC_SEG_FORWARD) ch = store.at(abg::MC_PAD + g.src + d);
			else if (g.kind == abg::MC_SEG_CONSENSUS) ch = sidebuf.at(g.src + d);
			else if (g.kind == abg::MC_SEG_REVERSE) ch = abg::ov_complement(store.at(abg::MC_PAD + g.src - d));
			else ch = (uint8_t)g.src;
			out[pos] = ch;
			counts[g.path] += abg::mc_acgt(ch) ? 1 : 0;
		}
	}

	std::string seq, log, err;
	for (uint64_t i = 0; i < np; ++i) {
		const Path& p = paths[i];
		if (p.flag) { // the product merges such a path on the host
			if (!abg::mc_merge_path_host(st, k, nodes.data() + noff[i], ov.data() + noff[i], noff[i + 1] - noff[i], 0, seq, log, err)) {
				fprintf(stderr, "mc_check: path %llu: %s\n", (unsigned long long)i, err.c_str());
				return 1;
			}
			counts[i] = (uint64_t)std::count_if(seq.begin(), seq.end(), [](char c) { return abg::mc_acgt((uint8_t)c); });
		} else seq.assign(out.begin() + p.at, out.begin() + p.at + p.length);
		printf("%s %d %llu\n", seq.c_str(), p.flag, (unsigned long long)counts[i]);
	}
	printf("# segments %llu %llu %llu %llu two-part gaps %llu\n", (unsigned long long)kinds[0], (unsigned long long)kinds[1], (unsigned long long)kinds[2],
	    (unsigned long long)kinds[3], (unsigned long long)two_part);
	return 0;
}

} // namespace

int main(int argc, char** argv)
{
	const std::string mode = argc > 1 ? argv[1] : "";
	if (mode == "run") {
		SerialMerger m;
		argv[1] = argv[0];
		return mc::run_main(argc - 1, argv + 1, m);
	}
	if (mode == "splice" && argc == 3) return splice(argv[2]);
	fprintf(stderr, "usage: mc_check run ARGS... | mc_check splice FILE\n");
	return 2;
}
