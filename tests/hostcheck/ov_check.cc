// ov_check -- Overlap without a GPU, for the CPU suite: the same overlap_core.h as abyss_amd/bin/Overlap over the search body of
// abg_ov.h run serially (what the kernel must equal).
//   ov_check run ARGS...      what `Overlap ARGS...` writes (stdout, the -o and -g files, stderr, status)
//   ov_check find PAIRS OUT   both modes of the search for a pair file
// A pair file, little-endian: u64 ncontigs, u64 offsets[n + 1], the bytes, u64 npairs, {u32 t, h}[npairs]; contigs are taken as
// they are (case already folded).  The result file: per pair u32 top[3], u32 ntop, u32 nall, u32 all[nall].
#include "../../abyss_amd/csrc/abg_ov.h"
#include "../../abyss_amd/csrc/host/overlap_core.h"

namespace {

// the store as abg_ov_set_contigs lays it out, with the reverse complements from the same table
struct SerialSearcher : ov::Searcher {
	std::vector<uint64_t> words, off;
	uint64_t total = 0;
	bool open(std::string&) override { return true; }
	bool set_contigs(const std::string& bytes, const std::vector<uint64_t>& offsets, std::string& err) override
	{
		off = offsets;
		total = bytes.size();
		words.assign((2 * total + 7) / 8 + abg::OV_PAD / 8, 0);
		uint8_t* s = (uint8_t*)words.data();
		memcpy(s, bytes.data(), total);
		for (size_t c = 0; c + 1 < off.size(); ++c)
			for (uint64_t i = off[c]; i < off[c + 1]; ++i) {
				const uint8_t x = abg::ov_complement(s[i]);
				if (!x) { err = "contig " + std::to_string(c) + ": unexpected character"; return false; }
				s[total + off[c] + (off[c + 1] - 1 - i)] = x;
			}
		return true;
	}
	abg::OVJob job(ov::V t, ov::V h) const
	{
		abg::OVJob j;
		j.tpos = (t & 1) * total + off[t >> 1];
		j.hpos = (h & 1) * total + off[h >> 1];
		j.tlen = (uint32_t)(off[(t >> 1) + 1] - off[t >> 1]);
		j.hlen = (uint32_t)(off[(h >> 1) + 1] - off[h >> 1]);
		j.bits = 0;
		return j;
	}
	bool find(const std::vector<std::pair<ov::V, ov::V>>& pairs, bool all, std::vector<uint32_t>& top, std::vector<uint32_t>& ntop,
	    std::vector<uint64_t>& all_offsets, std::vector<uint32_t>& lengths, std::string& err) override
	{
		top.assign(3 * pairs.size(), 0);
		ntop.assign(pairs.size(), 0);
		all_offsets.assign(1, 0);
		lengths.clear();
		std::vector<uint64_t> bits;
		for (size_t i = 0; i < pairs.size(); ++i) {
			if ((pairs[i].first >> 1) + 1 >= off.size() || (pairs[i].second >> 1) + 1 >= off.size()) { err = "no such contig"; return false; }
			const abg::OVJob j = job(pairs[i].first, pairs[i].second);
			if (all) {
				bits.assign(abg::ov_steps(j.tlen, j.hlen), 0);
				abg::ov_search_pair(words.data(), j, abg::OV_ALL, nullptr, nullptr, bits.data(), 0);
				abg::ov_expand(bits.data(), j.tlen, j.hlen, lengths);
				all_offsets.push_back(lengths.size());
			} else
				abg::ov_search_pair(words.data(), j, abg::OV_TOP, &top[3 * i], &ntop[i], nullptr, 0);
		}
		return true;
	}
};

template <class T> bool get(FILE* f, std::vector<T>& v, size_t n) { v.resize(n); return n == 0 || fread(v.data(), sizeof(T), n, f) == n; }

int find(const char* in, const char* out)
{
	FILE* f = fopen(in, "rb");
	if (!f) { fprintf(stderr, "ov_check: cannot read %s\n", in); return 2; }
	uint64_t n = 0, np = 0;
	std::vector<uint64_t> off;
	std::vector<char> bytes;
	std::vector<std::pair<ov::V, ov::V>> pairs;
	bool ok = fread(&n, 8, 1, f) == 1 && get(f, off, n + 1);
	ok = ok && get(f, bytes, off[n]) && fread(&np, 8, 1, f) == 1 && get(f, pairs, np);
	fclose(f);
	if (!ok) { fprintf(stderr, "ov_check: %s is cut short\n", in); return 2; }
	SerialSearcher s;
	std::string err;
	std::vector<uint32_t> top, ntop, lengths, t2, n2;
	std::vector<uint64_t> aoff, a2;
	if (!s.set_contigs(std::string(bytes.begin(), bytes.end()), off, err) || !s.find(pairs, false, top, ntop, a2, t2, err)
	    || !s.find(pairs, true, t2, n2, aoff, lengths, err)) {
		fprintf(stderr, "ov_check: %s\n", err.c_str());
		return 2;
	}
	FILE* o = fopen(out, "wb");
	if (!o) { fprintf(stderr, "ov_check: cannot write %s\n", out); return 2; }
	for (size_t i = 0; i < pairs.size(); ++i) {
		const uint32_t nall = (uint32_t)(aoff[i + 1] - aoff[i]);
		fwrite(&top[3 * i], 4, 3, o);
		fwrite(&ntop[i], 4, 1, o);
		fwrite(&nall, 4, 1, o);
		if (nall) fwrite(&lengths[aoff[i]], 4, nall, o);
	}
	return fclose(o) == 0 ? 0 : 2;
}

} // namespace

int main(int argc, char** argv)
{
	const std::string mode = argc > 1 ? argv[1] : "";
	if (mode == "run") {
		SerialSearcher s;
		argv[1] = argv[0];
		return ov::run_main(argc - 1, argv + 1, s);
	}
	if (mode == "find" && argc == 4) return find(argv[2], argv[3]);
	fprintf(stderr, "usage: ov_check run ARGS... | find PAIRS OUT\n");
	return 2;
}
