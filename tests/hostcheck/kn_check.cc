// kn_check.cc -- the host restatement of the Konnector filter (abyss_amd/csrc/abg_kn.h compiled by g++), for the tests.
//   kn_check hash                                   lines "k seed seq" on stdin -> the hash of every window, "-" where the
//                                                   window is not all ACGT (the known-answer vectors' format)
//   kn_check build K SEED LEVELS BITS START END OUT READS...
//                                                   the cascade filled one k-mer at a time, the last level written as a
//                                                   filter file
//   kn_check kmers K FILTER READS [fasta|bed|raw] [inverse]
//                                                   bloom.cc memberOf, one probe at a time
#include "../../abyss_amd/csrc/abg_kn.h"
#include "../../abyss_amd/csrc/host/bloom_core.h"
#include "../../abyss_amd/csrc/host/fasta_reader.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

static int hash_cmd()
{
	unsigned k;
	unsigned long long seed;
	std::string seq;
	while (std::cin >> k >> seed >> seq) {
		const abg::KnParams p = abg::make_kn_params(k, seed, 1, 1, 0, 0);
		std::string line;
		for (size_t i = 0; i + k <= seq.size(); i++) {
			bool ok = true;
			for (size_t j = i; j < i + k && ok; j++) ok = abg::kn_code((unsigned char)seq[j]) >= 0;
			if (i) line += ' ';
			line += ok ? std::to_string(abg::kn_hash_ascii(p, seq.data() + i)) : std::string("-");
		}
		puts(line.c_str());
	}
	return 0;
}

static int build_cmd(int argc, char** argv)
{
	if (argc < 10) return 2;
	const unsigned k = (unsigned)atoi(argv[2]), levels = (unsigned)atoi(argv[4]);
	const uint64_t seed = strtoull(argv[3], nullptr, 10), bits = strtoull(argv[5], nullptr, 10);
	const uint64_t start = strtoull(argv[6], nullptr, 10), end = strtoull(argv[7], nullptr, 10);
	const abg::KnParams p = abg::make_kn_params(k, seed, bits, levels, start, end);
	const uint64_t bytes = (end - start + 1 + 7) / 8;
	std::vector<std::vector<uint8_t>> lv(levels, std::vector<uint8_t>(bytes, 0));
	std::vector<uint8_t*> ptr;
	for (auto& l : lv) ptr.push_back(l.data());
	abghost::ReaderOptions ro;
	std::string id, comment, seq;
	for (int i = 9; i < argc; i++) {
		abghost::FastaReader in(argv[i], ro);
		while (in.read(id, comment, seq))
			abg::kn_host_windows(p, seq.data(), seq.size(), [&](uint64_t at) {
				abg::kn_host_insert(p, ptr.data(), abg::mod64(p.mod, abg::kn_hash_ascii(p, seq.data() + at)));
			});
	}
	FILE* f = fopen(argv[8], "wb");
	if (!f) return 1;
	kn::write_header(f, k, bits, start, end, seed);
	fwrite(lv.back().data(), 1, bytes, f);
	fclose(f);
	return 0;
}

static int kmers_cmd(int argc, char** argv)
{
	if (argc < 5) return 2;
	const unsigned k = (unsigned)atoi(argv[2]);
	const std::string fmt = argc > 5 ? argv[5] : "fasta";
	const bool inverse = argc > 6 && !strcmp(argv[6], "inverse");
	const kn::Format format = fmt == "bed" ? kn::BED : fmt == "raw" ? kn::RAW : kn::FASTA;
	FILE* f = fopen(argv[3], "rb");
	if (!f) return 1;
	const kn::Header h = kn::read_header(f, argv[3], k);
	std::vector<uint8_t> a((h.full + 7) / 8 + 1, 0);
	kn::load_bits(f, argv[3], h, a.data(), h.start, kn::OVERWRITE);
	fclose(f);
	const abg::KnParams p = abg::make_kn_params(k, h.seed, h.full, 1, 0, h.full - 1);
	abghost::ReaderOptions ro;
	abghost::FastaReader in(argv[4], ro);
	std::string id, comment, seq, out;
	for (uint64_t n = 0; in.read(id, comment, seq); n++) {
		out.clear();
		abg::kn_host_windows(p, seq.data(), seq.size(), [&](uint64_t at) {
			const uint64_t i = abg::mod64(p.mod, abg::kn_hash_ascii(p, seq.data() + at));
			const bool in_filter = (a[i / 8] >> (7 - i % 8)) & 1;
			if (in_filter != inverse) kn::format_kmer(out, format, id, n, at, k, seq.data() + at);
		});
		fwrite(out.data(), 1, out.size(), stdout);
	}
	return 0;
}

int main(int argc, char** argv)
{
	if (argc >= 2 && !strcmp(argv[1], "hash")) return hash_cmd();
	if (argc >= 2 && !strcmp(argv[1], "build")) return build_cmd(argc, argv);
	if (argc >= 2 && !strcmp(argv[1], "kmers")) return kmers_cmd(argc, argv);
	fprintf(stderr, "usage: kn_check hash | build K SEED LEVELS BITS START END OUT READS... | kmers K FILTER READS [fmt] [inverse]\n");
	return 2;
}
