// fm_check -- the CPU check of abyss-map / abyss-index: runs the serial bodies of abyss_amd/csrc/abg_fm.h (table build, search,
// locate) over a suffix array made by a plain host sort (test code only), and prints .fm, .fai and SAM through map_core.h.
//   fm_check map [abyss-map arguments]      fm_check index [abyss-index arguments]
//   fm_check hits K FLAGS TARGET READS      one line per read: both strands' l u qstart qend num pos
#include "../../abyss_amd/csrc/abg_fm.h"
#include "../../abyss_amd/csrc/host/map_core.h"

#include <algorithm>

namespace {

struct VecMemo {
	std::vector<uint64_t> e;
	uint32_t high = 0;
	void get(uint32_t j, uint32_t& l, uint32_t& u) const { l = (uint32_t)(e[j] >> 32); u = (uint32_t)e[j]; }
	void set(uint32_t j, uint32_t l, uint32_t u) { e[j] = ((uint64_t)l << 32) | u; if (j >= high) high = j + 1; }
	void reset() { std::fill(e.begin(), e.begin() + high, 0); high = 0; }
};

struct HostBackend : abgmap::Backend {
	std::vector<uint32_t> sa;
	std::vector<uint8_t> bwt; // 0..4, FM_SENT
	std::vector<abg::FMBlock> occ;
	abg::FMView v{};
	bool build(const uint8_t* text, uint64_t n, std::string& err) override
	{
		if (n == 0 || n >= 0xFFFFFFFFull) { err = "bad text size"; return false; }
		std::vector<uint8_t> t(n);
		for (uint64_t i = 0; i < n; i++) t[i] = (uint8_t)abg::fm_text_code(text[i]);
		sa.resize(n + 1);
		sa[0] = (uint32_t)n;
		for (uint64_t i = 0; i < n; i++) sa[i + 1] = (uint32_t)i;
		std::sort(sa.begin() + 1, sa.end(), [&](uint32_t a, uint32_t b) {
			const size_t la = n - a, lb = n - b;
			const int c = memcmp(&t[a], &t[b], std::min(la, lb));
			return c ? c < 0 : la < lb;
		});
		const uint32_t m = (uint32_t)n + 1, nb = m / abg::FM_BLOCK + 1;
		bwt.resize(m);
		for (uint32_t i = 0; i < m; i++) {
			bwt[i] = sa[i] == 0 ? (uint8_t)abg::FM_SENT : t[sa[i] - 1];
			if (sa[i] == 0) v.sent = i;
		}
		occ.resize(nb);
		uint32_t run[4] = { 0, 0, 0, 0 };
		for (uint32_t b = 0; b < nb; b++) {
			uint32_t local[4];
			abg::fm_fill_block(bwt.data(), m, b, occ[b], local);
			for (int c = 0; c < 4; c++) { occ[b].cnt[c] = run[c]; run[c] += local[c]; }
		}
		v.occ = occ.data();
		v.m = m;
		v.cf[0] = 1;
		v.cf[1] = 1 + ((uint32_t)n - run[0] - run[1] - run[2] - run[3]);
		for (int c = 1; c < 4; c++) v.cf[c + 1] = v.cf[c] + run[c - 1];
		return true;
	}
	bool exported(std::vector<uint32_t>& s, std::vector<uint8_t>& b, std::string&) override
	{
		s = sa;
		b = bwt;
		for (auto& c : b) if (c == abg::FM_SENT) c = 255;
		return true;
	}
	bool map(const char* seqs, const uint64_t* off, uint64_t n, uint32_t k, uint32_t flags, abgmap::Hit* out, std::string&) override
	{
		static_assert(sizeof(abgmap::Hit) == sizeof(abg::FMHit), "one layout");
		VecMemo memo;
		for (uint64_t i = 0; i < n; i++) {
			const unsigned char* s = (const unsigned char*)seqs + off[i];
			const uint32_t L = (uint32_t)(off[i + 1] - off[i]);
			if (memo.e.size() < L) memo.e.resize(L, 0);
			abg::fm_map_read(v, sa.data(), [&](uint32_t j) { return (unsigned)s[j]; }, L, k, flags, memo, (abg::FMHit*)out + 2 * i);
			memo.reset();
		}
		return true;
	}
};

abgmap::Backend* make_host(std::string&) { return new HostBackend; }

int hits_main(int argc, char** argv)
{
	if (argc != 5) { fprintf(stderr, "usage: fm_check hits K FLAGS TARGET READS\n"); return 2; }
	std::string text, err;
	if (!abgmap::read_file(argv[3], text)) abgmap::die_io(argv[3]);
	HostBackend be;
	if (!be.build((const uint8_t*)text.data(), text.size(), err)) { fprintf(stderr, "fm_check: %s\n", err.c_str()); return 1; }
	abghost::ReaderOptions ro;
	ro.chastityFilter = 0; ro.trimMasked = 0; ro.foldCase = 1;
	abgmap::Interleave in({ argv[4] }, ro);
	abgmap::Block b;
	abgmap::read_block(in, (size_t)-1, (size_t)-1, b);
	std::vector<abgmap::Hit> h(2 * b.recs.size());
	be.map(b.seqs.data(), b.off.data(), b.recs.size(), (uint32_t)atoi(argv[1]), (uint32_t)atoi(argv[2]), h.data(), err);
	for (size_t i = 0; i < h.size(); i += 2)
		printf("%u %u %u %u %u %u %u %u %u %u %u %u\n", h[i].l, h[i].u, h[i].qstart, h[i].qend, h[i].num, h[i].pos, h[i + 1].l, h[i + 1].u, h[i + 1].qstart,
		    h[i + 1].qend, h[i + 1].num, h[i + 1].pos);
	return 0;
}

} // namespace

int main(int argc, char** argv)
{
	if (argc >= 2 && !strcmp(argv[1], "map")) { argv[1] = (char*)"abyss-map"; return abgmap::map_main(argc - 1, argv + 1, make_host); }
	if (argc >= 2 && !strcmp(argv[1], "index")) { argv[1] = (char*)"abyss-index"; return abgmap::index_main(argc - 1, argv + 1, make_host); }
	if (argc >= 2 && !strcmp(argv[1], "hits")) return hits_main(argc - 1, argv + 1);
	fprintf(stderr, "usage: fm_check map|index|hits ...\n");
	return 2;
}
