// bloom_main.cc -- `abyss-bloom build` on the MI355X: the two Bloom-filter builders of the
// reference's Bloom/bloom.cc that share the abyss-bloom-dbg hot path,
//   build -t counting      (bloom.cc:605-620)  -> [BTLCountingBloomFilter_v1] file for abyss-bloom-dbg -i
//   build -t rolling-hash  (bloom.cc:585-602)  -> last level of a HashAgnosticCascadingBloom,
//                                                [BTLBloomFilter_v1] file
// over the C ABI (include/abyss_amd.h); and the Konnector filters and the commands on their files
//   build -t konnector     (bloom.cc:522-581, the default type) -> CascadingBloomFilter[Window], the kernels of abg_kn.hip
//   union / intersect      (bloom.cc:766-821)   host-side file streaming (bloom_core.h): the HIP runtime is never started
//   info                   (bloom.cc:822-847)   "
//   compare                (bloom.cc:849-977)   "  (status 1, as the reference's)
//   kmers / getKmers       (bloom.cc:1155-1234) the probes on the GPU, the output formatted on up to 16 threads, in order
// `graph' and `trim' (a DBGBloom walk) are not provided by this build.
#include "../../../include/abyss_amd.h"
#include "bloom_core.h"
#include "fasta_reader.h"
#include "si_bytes.h"

#include <iostream>

#include <algorithm>
#include <thread>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <getopt.h>
#include <string>
#include <vector>

#define PROGRAM "abyss-bloom"

static abghost::ReaderOptions ropt;
static const struct option longopts[] = {
	{ "bloom-size", required_argument, NULL, 'b' }, { "threads", required_argument, NULL, 'j' },
	{ "kmer", required_argument, NULL, 'k' }, { "num-hashes", required_argument, NULL, 'H' },
	{ "levels", required_argument, NULL, 'l' }, { "chastity", no_argument, &ropt.chastityFilter, 1 },
	{ "no-chastity", no_argument, &ropt.chastityFilter, 0 }, { "trim-masked", no_argument, &ropt.trimMasked, 1 },
	{ "no-trim-masked", no_argument, &ropt.trimMasked, 0 }, { "trim-quality", required_argument, NULL, 'q' },
	{ "bloom-type", required_argument, NULL, 't' }, { "standard-quality", no_argument, &ropt.qualityOffset, 33 },
	{ "illumina-quality", no_argument, &ropt.qualityOffset, 64 }, { "verbose", no_argument, NULL, 'v' },
	{ NULL, 0, NULL, 0 }
};

static void check(int rc, abg_ctx* ctx, const char* what)
{
	if (rc == ABG_OK) return;
	fprintf(stderr, PROGRAM ": %s: %s\n", what, abg_last_error(ctx));
	exit(EXIT_FAILURE);
}

static int build_btl(int argc, char** argv)
{
	optind = 2;
	uint64_t bloomSize = 500ull << 20; // bloom.cc: default 500M
	unsigned k = 0, H = 1, levels = 1;
	std::string type = "konnector";
	int verbose = 0;
	for (int c; (c = getopt_long(argc, argv, "b:B:j:k:H:l:q:t:v", longopts, NULL)) != -1;) {
		switch (c) {
		case 'b': if (!si_to_bytes(optarg, &bloomSize)) { fprintf(stderr, PROGRAM ": invalid option: `-b%s'\n", optarg); return EXIT_FAILURE; } break;
		case 'k': k = (unsigned)atoi(optarg); break;
		case 'H': H = (unsigned)atoi(optarg); break;
		case 'l': levels = (unsigned)atoi(optarg); break;
		case 'q': ropt.qualityThreshold = atoi(optarg); break;
		case 't': type = optarg; break;
		case 'v': verbose++; break;
		case 'B': case 'j': break;
		case '?': return EXIT_FAILURE;
		}
	}
	if (k == 0) { fprintf(stderr, PROGRAM ": missing mandatory option `-k'\n"); return EXIT_FAILURE; }
	if (type == "counting" && levels > 1) { fprintf(stderr, PROGRAM ": `-l' is not supported when using `-t counting'\n"); return EXIT_FAILURE; }
	if (argc - optind < 2) { fprintf(stderr, PROGRAM ": missing arguments\n"); return EXIT_FAILURE; }
	std::string outputPath = argv[optind++];

	abg_params p;
	abg_params_init(&p);
	p.k = k; p.num_hashes = H; p.min_cov = 0; p.verbose = verbose;
	if (type == "counting") {
		p.counters = bloomSize; // CountingBloomFilter<uint8_t>(bytes, H, k, 0), bloom.cc:610
	} else {
		uint64_t bits = bloomSize * 8 / levels; // roundUpToMultiple(bits / levels, 64), bloom.cc:590
		if (bits % 64) bits += 64 - bits % 64;
		p.counters = bits;
		p.cascade_levels = levels;
	}
	abg_ctx* ctx = NULL;
	if (abg_create(&p, &ctx) != ABG_OK) { fprintf(stderr, PROGRAM ": %s\n", abg_last_error(NULL)); return EXIT_FAILURE; }
	uint64_t size = 0;
	abg_filter_size(ctx, &size);
	std::string id, comment, seq, seqs;
	std::vector<uint64_t> off{ 0 };
	for (int i = optind; i < argc; i++) { // BloomDBG::loadFile for each file, bloom.cc:596-597,613-614
		if (verbose) fprintf(stderr, "Reading `%s'...\n", argv[i]);
		abghost::SequenceReader in(argv[i], ropt, std::min(16u, std::max(1u, std::thread::hardware_concurrency())));
		while (in.read(id, comment, seq)) {
			seqs += seq; off.push_back(seqs.size());
			if (seqs.size() >= (256u << 20)) { check(abg_load_seqs(ctx, seqs.data(), off.data(), off.size() - 1), ctx, "load"); seqs.clear(); off.assign(1, 0); }
		}
		if (off.size() > 1) { check(abg_load_seqs(ctx, seqs.data(), off.data(), off.size() - 1), ctx, "load"); seqs.clear(); off.assign(1, 0); }
	}
	FILE* f = fopen(outputPath.c_str(), "wb");
	if (!f) { fprintf(stderr, "error: `%s': %s\n", outputPath.c_str(), strerror(errno)); return EXIT_FAILURE; }
	if (type == "counting") {
		// CountingBloomFilter::storeHeader + raw counters (CountingBloomFilter.hpp:344-379), key order as cpptoml emits it
		std::vector<uint8_t> cnt(size);
		check(abg_counters_export(ctx, cnt.data()), ctx, "export");
		fprintf(stderr, "Writing a %llu byte filter to %s on disk.\n", (unsigned long long)size, outputPath.c_str());
		fprintf(f, "[BTLCountingBloomFilter_v1]\n\tBloomFilterSize = %llu\n\tHashNum = %u\n\tKmerSize = %u\n"
		           "\tBloomFilterSizeInBytes = %llu\n\tBitsPerCounter = 8\n[HeaderEnd]\n",
		    (unsigned long long)size, H, k, (unsigned long long)size);
		fwrite(cnt.data(), 1, cnt.size(), f);
	} else {
		// operator<< of the last level (HashAgnosticCascadingBloom.h:143-150; BloomFilter::writeHeader, BloomFilter.hpp:261-294)
		std::vector<uint8_t> bits(size / 8);
		check(abg_cascade_export(ctx, levels - 1, bits.data()), ctx, "export");
		fprintf(f, "[BTLBloomFilter_v1]\n\tnEntry = 0\n\tdFPR = 0.0000000000000000\n\tEntry = 0\n"
		           "\tBloomFilterSizeInBytes = %llu\n\tBloomFilterSize = %llu\n\tHashNum = %u\n\tKmerSize = %u\n[HeaderEnd]\n",
		    (unsigned long long)(size / 8), (unsigned long long)size, H, k);
		fwrite(bits.data(), 1, bits.size(), f);
	}
	fclose(f);
	abg_destroy(ctx);
	return EXIT_SUCCESS;
}

// ---- Konnector filters and the commands on their files -------------------------------------------------------------------

enum { OPT_HELP = 1, OPT_VERSION, OPT_BED, OPT_FASTA, OPT_RAW };
static const char kn_shortopts[] = "a:A:b:B:d:f:h:H:j:k:l:L:m:n:q:rR:vt:w:";
static const struct option kn_longopts[] = {
	{ "bloom-size", required_argument, NULL, 'b' }, { "bloom-type", required_argument, NULL, 't' },
	{ "buffer-size", required_argument, NULL, 'B' }, { "hash-seed", required_argument, NULL, 'h' },
	{ "num-hashes", required_argument, NULL, 'H' }, { "threads", required_argument, NULL, 'j' },
	{ "kmer", required_argument, NULL, 'k' }, { "levels", required_argument, NULL, 'l' },
	{ "init-level", required_argument, NULL, 'L' }, { "chastity", no_argument, &ropt.chastityFilter, 1 },
	{ "no-chastity", no_argument, &ropt.chastityFilter, 0 }, { "trim-masked", no_argument, &ropt.trimMasked, 1 },
	{ "no-trim-masked", no_argument, &ropt.trimMasked, 0 }, { "num-locks", required_argument, NULL, 'n' },
	{ "trim-quality", required_argument, NULL, 'q' }, { "standard-quality", no_argument, &ropt.qualityOffset, 33 },
	{ "illumina-quality", no_argument, &ropt.qualityOffset, 64 }, { "verbose", no_argument, NULL, 'v' },
	{ "help", no_argument, NULL, OPT_HELP }, { "version", no_argument, NULL, OPT_VERSION },
	{ "window", required_argument, NULL, 'w' }, { "method", required_argument, NULL, 'm' },
	{ "inverse", no_argument, NULL, 'r' }, { "bed", no_argument, NULL, OPT_BED }, { "fasta", no_argument, NULL, OPT_FASTA },
	{ "raw", no_argument, NULL, OPT_RAW }, { NULL, 0, NULL, 0 }
};

static const char USAGE[] =
    "Usage 1: " PROGRAM " build [GLOBAL_OPTS] [COMMAND_OPTS] <OUTPUT_BLOOM_FILE> <READS_FILE_1> [READS_FILE_2]...\n"
    "Usage 2: " PROGRAM " union [GLOBAL_OPTS] [COMMAND_OPTS] <OUTPUT_BLOOM_FILE> <BLOOM_FILE_1> <BLOOM_FILE_2> [BLOOM_FILE_3]...\n"
    "Usage 3: " PROGRAM " intersect [GLOBAL_OPTS] [COMMAND_OPTS] <OUTPUT_BLOOM_FILE> <BLOOM_FILE_1> <BLOOM_FILE_2> [BLOOM_FILE_3]...\n"
    "Usage 4: " PROGRAM " info [GLOBAL_OPTS] [COMMAND_OPTS] <BLOOM_FILE>\n"
    "Usage 5: " PROGRAM " compare [GLOBAL_OPTS] [COMMAND_OPTS] <BLOOM_FILE_1> <BLOOM_FILE_2>\n"
    "Usage 8: " PROGRAM " kmers [GLOBAL_OPTS] [COMMAND_OPTS] <BLOOM_FILE> <READS_FILE>\n"
    "\n"
    "Build and manipulate Bloom filter files on the GPU (`graph' and `trim' are not provided by this build).\n"
    "\n"
    " Global options:\n"
    "  -k, --kmer=N               the size of a k-mer [<=192]\n"
    "  -v, --verbose              display verbose output\n"
    "      --help                 display this help and exit\n"
    " Options for `" PROGRAM " build':\n"
    "  -b, --bloom-size=N         size of bloom filter [500M]\n"
    "  -B, --buffer-size=N        accepted and ignored\n"
    "  -j, --threads=N            parser threads, at most 16 [1]\n"
    "  -h, --hash-seed=N          seed for hash function (only works with `-t konnector') [0]\n"
    "  -H, --num-hashes=N         number of hash functions (only works with `-t rolling-hash') [1]\n"
    "  -l, --levels=N             build a cascading bloom filter with N levels and output the last level\n"
    "  -L, --init-level='N=FILE'  initialize level N of cascading bloom filter from FILE\n"
    "      --chastity / --no-chastity, --trim-masked / --no-trim-masked, -q, --trim-quality=N,\n"
    "      --standard-quality, --illumina-quality   as in the reference\n"
    "  -n, --num-locks=N          accepted and ignored\n"
    "  -t, --bloom-type=STR       'konnector', 'rolling-hash', or 'counting' [konnector]\n"
    "  -w, --window M/N           build a bloom filter for subwindow M of N\n"
    " Options for `" PROGRAM " compare':\n"
    "  -m, --method=`String'      `jaccard' (default), `forbes', `czekanowski'\n"
    " Options for `" PROGRAM " kmers':\n"
    "  -r, --inverse              get k-mers that are *NOT* in the bloom filter\n"
    "  --bed / --fasta / --raw    output format [fasta]\n";

[[noreturn]] static void usage_error()
{
	fputs("Try `" PROGRAM " --help' for more information.\n", stderr);
	exit(EXIT_FAILURE);
}

struct KnOpts {
	unsigned k = 0, levels = 1, H = 1, threads = 1, windows = 0, window = 0;
	uint64_t bloomSize = 500ull << 20, seed = 0;
	int verbose = 0, inverse = 0;
	std::string type = "konnector", method = "jaccard";
	std::vector<std::vector<std::string>> levelInit;
	kn::Format format = kn::FASTA;
};

static bool parse_u64(const char* s, uint64_t* v)
{
	char* end;
	if (!*s || *s == '-') return false;
	errno = 0;
	*v = strtoull(s, &end, 10);
	return !*end && !errno;
}

// every option of every command in one pass (the reference parses the global ones first, then the command's)
static KnOpts parse_opts(int argc, char** argv)
{
	KnOpts o;
	optind = 2;
	for (int c; (c = getopt_long(argc, argv, kn_shortopts, kn_longopts, NULL)) != -1;) {
		uint64_t v = 0;
		bool bad = false;
		switch (c) {
		case '?': usage_error();
		case OPT_HELP: fputs(USAGE, stdout); exit(EXIT_SUCCESS);
		case OPT_VERSION: puts(PROGRAM " (abyss_amd)"); exit(EXIT_SUCCESS);
		case 'k': bad = !parse_u64(optarg, &v); o.k = (unsigned)v; break;
		case 'v': o.verbose++; break;
		case 'b': bad = !si_to_bytes(optarg, &o.bloomSize); break;
		case 'h': bad = !parse_u64(optarg, &o.seed); break;
		case 'H': bad = !parse_u64(optarg, &v); o.H = (unsigned)v; break;
		case 'j': bad = !parse_u64(optarg, &v); o.threads = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(16, v)); break;
		case 'l': bad = !parse_u64(optarg, &v); o.levels = (unsigned)v; break;
		case 'L': {
			const char* eq = strchr(optarg, '=');
			std::string lv = eq ? std::string(optarg, eq - optarg) : std::string();
			if (!eq || !parse_u64(lv.c_str(), &v) || v == 0 || !eq[1]) break; // (bloom.cc:653-665: ignored when it does not parse)
			if (v > o.levelInit.size()) o.levelInit.resize(v);
			o.levelInit[v - 1].push_back(eq + 1);
			break;
		}
		case 'q': bad = !parse_u64(optarg, &v); ropt.qualityThreshold = (int)v; break;
		case 't': o.type = optarg; break;
		case 'w': {
			unsigned m = 0, n = 0;
			char tail;
			bad = sscanf(optarg, "%u/%u%c", &m, &n, &tail) != 2;
			o.window = m; o.windows = n;
			break;
		}
		case 'm': o.method = optarg; break;
		case 'r': o.inverse = 1; break;
		case OPT_BED: o.format = kn::BED; break;
		case OPT_FASTA: o.format = kn::FASTA; break;
		case OPT_RAW: o.format = kn::RAW; break;
		default: break; // -B -n -a -A -d -f -R, the reader flags
		}
		if (bad) { fprintf(stderr, PROGRAM ": invalid option: `-%c%s'\n", c, optarg); exit(EXIT_FAILURE); }
	}
	if (o.k == 0) { fprintf(stderr, PROGRAM ": missing mandatory option `-k'\n"); usage_error(); }
	if (o.k > 192u) {
		fprintf(stderr, "Error: k is %u and must be no more than %u. You can recompile ABySS to increase this limit.\n", o.k, 192u);
		exit(EXIT_FAILURE);
	}
	return o;
}

static FILE* open_in(const std::string& path)
{
	if (path == "-") return stdin;
	FILE* f = fopen(path.c_str(), "rb");
	if (!f) kn::die("error: `" + path + "': " + strerror(errno) + "\n");
	return f;
}
static void close_in(FILE* f) { if (f != stdin) fclose(f); }
static FILE* open_out(const std::string& path)
{
	if (path == "-") return stdout;
	FILE* f = fopen(path.c_str(), "wb");
	if (!f) kn::die("error: `" + path + "': " + strerror(errno) + "\n");
	return f;
}
static void close_out(FILE* f, const std::string& path)
{
	if (fflush(f) != 0 || ferror(f)) kn::die("error: `" + path + "': " + strerror(errno) + "\n");
	if (f != stdout) fclose(f);
}

// A full-size Konnector::BloomFilter on the host (union, intersect, info, kmers): bits, seed, the byte array (+1 byte that
// read_bits may touch past the end)
struct HostFilter {
	uint64_t size = 0, seed = 0;
	std::vector<uint8_t> a;
	// Konnector::BloomFilter::read(in, op)
	void read(const std::string& path, unsigned k, kn::Op op)
	{
		FILE* f = open_in(path);
		const kn::Header h = kn::read_header(f, path, k);
		if (seed != h.seed) {
			if (op != kn::OVERWRITE) kn::die("error: can't union/intersect bloom filters with different hash seeds\n");
			seed = h.seed;
		}
		if (size != h.full) {
			if (op != kn::OVERWRITE) kn::die("error: can't union/intersect bloom filters with different sizes\n");
			size = h.full;
			a.assign((size + 7) / 8 + 1, 0);
		}
		kn::load_bits(f, path, h, a.data(), h.start, op);
		close_in(f);
	}
	void write(const std::string& path, unsigned k) const
	{
		FILE* f = open_out(path);
		kn::write_header(f, k, size, 0, size - 1, seed);
		fwrite(a.data(), 1, (size + 7) / 8, f);
		close_out(f, path);
	}
	std::string stats() const { return kn::bloom_stats(size, kn::popcount(a.data(), size)); }
};

static void check_kn(int rc, abg_kn* f, const char* what)
{
	if (rc == ABG_OK) return;
	fprintf(stderr, PROGRAM ": %s: %s\n", what, abg_kn_last_error(f));
	exit(EXIT_FAILURE);
}

// bloom.cc buildKonnectorBloom
static int build_konnector(int argc, char** argv, const KnOpts& o)
{
	if (!o.levelInit.empty() && o.levels < 2) {
		fprintf(stderr, PROGRAM ": -L can only be used with cascading bloom filters (-l >= 2)\n");
		usage_error();
	}
	if (o.levelInit.size() > o.levels) {
		fprintf(stderr, PROGRAM ": level arg to -L is greater than number of bloom filter levels (-l)\n");
		usage_error();
	}
	if (o.H != 1) fprintf(stderr, PROGRAM ": warning: -H option has no effect when using `-t konnector'\n");
	if (o.levels == 0) { fprintf(stderr, PROGRAM ": invalid option: `-l0'\n"); return EXIT_FAILURE; }
	const uint64_t bits = o.bloomSize * 8;
	if (o.windows != 0 && bits / o.levels % o.windows != 0) {
		fprintf(stderr, PROGRAM ": (b / l) %% w == 0 must be true, where b is bloom filter size (-b), l is number of levels (-l), and w is number of windows (-w)\n");
		usage_error();
	}
	if (argc - optind < 2) { fprintf(stderr, PROGRAM ": missing arguments\n"); usage_error(); }
	const std::string outputPath = argv[optind++];
	if (o.verbose)
		fprintf(stderr, "Building a Bloom filter of type 'konnector' with %u level(s), 1 hash function(s), and a total size of %llu bytes\n",
		    o.levels, (unsigned long long)o.bloomSize);
	const uint64_t levelBits = bits / o.levels; // bloom.cc:528, no rounding
	if (levelBits == 0) { fprintf(stderr, PROGRAM ": the Bloom filter is too small\n"); return EXIT_FAILURE; }
	uint64_t start = 0, end = levelBits - 1;
	if (o.windows != 0) {
		if (o.window < 1 || o.window > o.windows) { fprintf(stderr, PROGRAM ": invalid option: `-w %u/%u'\n", o.window, o.windows); return EXIT_FAILURE; }
		const uint64_t per = levelBits / o.windows;
		start = (o.window - 1) * per;
		end = o.window < o.windows ? o.window * per - 1 : levelBits - 1;
	}
	const uint64_t winBits = end - start + 1, winBytes = (winBits + 7) / 8;
	uint64_t lastSeed = o.seed; // BloomFilter::read with a different seed takes the file's (what the last level's header says)

	// -L: every file read into a host copy of its level (BloomFilter::read / BloomFilterWindow::read), before any read is loaded
	std::vector<std::vector<uint8_t>> preset(o.levelInit.size());
	for (size_t i = 0; i < o.levelInit.size(); i++) {
		for (size_t j = 0; j < o.levelInit[i].size(); j++) {
			const std::string& path = o.levelInit[i][j];
			fprintf(stderr, "Loading `%s' into level %zu of cascading bloom filter...\n", path.c_str(), i + 1);
			FILE* f = open_in(path);
			const kn::Header h = kn::read_header(f, path, o.k);
			const kn::Op op = j > 0 ? kn::OR : kn::OVERWRITE;
			if (h.seed != o.seed && j == 0 && i + 1 == o.levels) lastSeed = h.seed;
			if (o.windows == 0) {
				if (h.full != levelBits) kn::die(PROGRAM ": `" + path + "': -L needs a filter of the level's size (" + std::to_string(levelBits) + " bits)\n");
				if (preset[i].empty()) preset[i].assign(winBytes + 1, 0);
				kn::load_bits(f, path, h, preset[i].data(), h.start, op);
			} else {
				if (h.start != start || h.end != end) kn::die(PROGRAM ": `" + path + "': -L needs a filter of the same window\n");
				if (preset[i].empty()) preset[i].assign(winBytes + 1, 0);
				kn::load_bits(f, path, h, preset[i].data(), 0, op);
			}
			close_in(f);
		}
	}

	abg_kn* kf = nullptr;
	if (abg_kn_create(0, levelBits, o.levels, o.k, o.seed, start, end, &kf) != ABG_OK) {
		fprintf(stderr, PROGRAM ": %s\n", abg_kn_last_error(NULL));
		return EXIT_FAILURE;
	}
	for (size_t i = 0; i < preset.size(); i++)
		if (!preset[i].empty()) check_kn(abg_kn_import(kf, (uint32_t)i, preset[i].data()), kf, "-L");

	// Bloom::loadFile for every file: the block reader parses ahead while the chunks go to the device
	std::string seqs, id, comment, seq;
	std::vector<uint64_t> off{ 0 };
	for (int i = optind; i < argc; i++) {
		if (o.verbose) fprintf(stderr, "Reading `%s'...\n", argv[i]);
		uint64_t count = 0;
		abghost::SequenceReader in(argv[i], ropt, o.threads);
		while (in.read(id, comment, seq)) {
			seqs += seq;
			off.push_back(seqs.size());
			if (o.verbose && ++count % 100000 == 0) fprintf(stderr, "Loaded %llu reads into bloom filter\n", (unsigned long long)count);
			if (seqs.size() >= (48u << 20)) {
				check_kn(abg_kn_insert_seqs(kf, seqs.data(), off.data(), off.size() - 1), kf, "load");
				seqs.clear();
				off.assign(1, 0);
			}
		}
		if (off.size() > 1) check_kn(abg_kn_insert_seqs(kf, seqs.data(), off.data(), off.size() - 1), kf, "load");
		seqs.clear();
		off.assign(1, 0);
		if (o.verbose) fprintf(stderr, "Loaded %llu reads from `%s` into bloom filter\n", (unsigned long long)count, argv[i]);
	}
	if (o.verbose) fputs("Successfully loaded bloom filter.\n", stderr);
	std::vector<uint64_t> pops(o.levels);
	check_kn(abg_kn_popcount(kf, pops.data()), kf, "popcount");
	fputs(o.levels == 1 ? kn::bloom_stats(winBits, pops[0]).c_str() : kn::cascading_stats(winBits, pops).c_str(), stderr);
	std::vector<uint8_t> last(winBytes);
	check_kn(abg_kn_export(kf, o.levels - 1, last.data()), kf, "export");
	abg_kn_destroy(kf);
	if (o.verbose) fprintf(stderr, "Writing bloom filter to `%s'...\n", outputPath.c_str());
	FILE* f = open_out(outputPath);
	kn::write_header(f, o.k, levelBits, start, end, lastSeed);
	fwrite(last.data(), 1, last.size(), f);
	close_out(f, outputPath);
	return EXIT_SUCCESS;
}

// bloom.cc combine
static int combine(int argc, char** argv, kn::Op op)
{
	const KnOpts o = parse_opts(argc, argv);
	if (argc - optind < 3) { fprintf(stderr, PROGRAM ": missing arguments\n"); usage_error(); }
	const std::string outputPath = argv[optind++];
	HostFilter bf;
	for (int i = optind; i < argc; i++) {
		if (o.verbose) fprintf(stderr, "Loading bloom filter from `%s'...\n", argv[i]);
		bf.read(argv[i], o.k, i > optind ? op : kn::OVERWRITE);
	}
	if (o.verbose) {
		fputs("Successfully loaded bloom filter.\n", stderr);
		fputs(bf.stats().c_str(), stderr);
		fprintf(stderr, "Writing %s of bloom filters to `%s'...\n", op == kn::OR ? "union" : "intersection", outputPath.c_str());
	}
	bf.write(outputPath, o.k);
	return EXIT_SUCCESS;
}

// bloom.cc info
static int info(int argc, char** argv)
{
	const KnOpts o = parse_opts(argc, argv);
	if (argc - optind < 1) { fprintf(stderr, PROGRAM ": missing arguments\n"); usage_error(); }
	const std::string path = argv[optind];
	if (o.verbose) fprintf(stderr, "Loading bloom filter from `%s'...\n", path.c_str());
	HostFilter bf;
	bf.read(path, o.k, kn::OVERWRITE);
	fputs(bf.stats().c_str(), stderr);
	return EXIT_SUCCESS;
}

// bloom.cc compare.  Counts exactly ceil(bits / 8) bytes of each file, all 8 bits of each byte (the reference counts its last
// 32 KB read buffer in full, whatever its fill: the same numbers whenever the size is a multiple of 262,144 bits).
static int compare(int argc, char** argv)
{
	const KnOpts o = parse_opts(argc, argv);
	if (o.method != "jaccard" && o.method != "czekanowski" && o.method != "forbes") std::cerr << "Invalid method: " << o.method << std::endl;
	if (argc - optind < 2) { fprintf(stderr, PROGRAM ": missing arguments\n"); usage_error(); }
	if (o.verbose) std::cerr << "Computing distance for 2 samples...\n";
	const std::string pathA = argv[optind], pathB = argv[optind + 1];
	if (o.verbose) std::cerr << "Loading bloom filters from " << pathA << " and " << pathB << "...\n";
	FILE* fa = open_in(pathA);
	FILE* fb = open_in(pathB);
	const kn::Header ha = kn::read_header(fa, pathA, o.k), hb = kn::read_header(fb, pathB, o.k);
	if (ha.bits() != hb.bits()) { std::cerr << "Bit sizes of arrays not equal" << std::endl; exit(EXIT_FAILURE); }
	if (o.verbose) std::cerr << "Bits: " << ha.bits() << std::endl;
	unsigned long a = 0, b = 0, c = 0, d = 0;
	std::vector<uint8_t> x(1u << 20), y(1u << 20);
	for (uint64_t left = ha.bytes(); left;) {
		const size_t n = (size_t)std::min<uint64_t>(left, x.size());
		if (fread(x.data(), 1, n, fa) != n) kn::die("error: `" + pathA + "': the Bloom filter file is truncated\n");
		if (fread(y.data(), 1, n, fb) != n) kn::die("error: `" + pathB + "': the Bloom filter file is truncated\n");
		for (size_t i = 0; i < n; i++) {
			const unsigned p = x[i], q = y[i];
			a += (unsigned)__builtin_popcount(p & q);
			b += (unsigned)__builtin_popcount(p & ~q & 0xFFu);
			c += (unsigned)__builtin_popcount(~p & q & 0xFFu);
			d += 8 - (unsigned)__builtin_popcount(p | q);
		}
		left -= n;
	}
	close_in(fa);
	close_in(fb);
	std::cout << "1/1: " << a << "\n1/0: " << b << "\n0/1: " << c << "\n0/0: " << d << std::endl;
	if (o.method == "jaccard") std::cout << "Jaccard similarity: " << (float)a / (float)(a + b + c) << std::endl;
	if (o.method == "czekanowski") std::cout << "Czekanowski similarity: " << (2 * (float)a) / (float)((2 * a) + b + c) << std::endl;
	if (o.method == "forbes") {
		const float n = (float)(a + b + c + d);
		const float dist = (n * a - ((a + b) * (a + c))) / (n * std::min(a + b, a + c) - ((a + b) * (a + c)));
		std::cout << "Forbes similarity: " << dist << std::endl;
	}
	return 1; // bloom.cc:976
}

// bloom.cc memberOf
static int kmers(int argc, char** argv)
{
	const KnOpts o = parse_opts(argc, argv);
	if (argc - optind < 2) { fprintf(stderr, PROGRAM ": missing arguments\n"); usage_error(); }
	const std::string path = argv[optind], fasta = argv[optind + 1];
	const unsigned k = o.k;
	if (o.verbose) fprintf(stderr, "Loading bloom filter from `%s'...\n", path.c_str());
	HostFilter bf;
	bf.read(path, k, kn::OVERWRITE);
	abg_kn* kf = nullptr;
	if (abg_kn_create(0, bf.size, 1, k, bf.seed, 0, bf.size - 1, &kf) != ABG_OK) {
		fprintf(stderr, PROGRAM ": %s\n", abg_kn_last_error(NULL));
		return EXIT_FAILURE;
	}
	check_kn(abg_kn_import(kf, 0, bf.a.data()), kf, "load");
	if (o.verbose) fprintf(stderr, "Reading `%s'...\n", fasta.c_str());
	const unsigned T = std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
	abghost::SequenceReader in(fasta, ropt, T);
	std::vector<std::string> ids;
	std::string seqs, id, comment, seq;
	std::vector<uint64_t> off{ 0 };
	std::vector<uint8_t> print;
	std::vector<std::string> outs(T);
	uint64_t seqCount = 0;
	bool more = true;
	while (more) {
		ids.clear(); seqs.clear(); off.assign(1, 0);
		while (seqs.size() < (32u << 20) && (more = in.read(id, comment, seq))) {
			ids.push_back(id);
			seqs += seq;
			off.push_back(seqs.size());
		}
		const uint64_t n = ids.size();
		if (n == 0) break;
		print.assign(seqs.size(), 0);
		check_kn(abg_kn_contains_seqs(kf, seqs.data(), off.data(), n, o.inverse, print.data()), kf, "probe");
		// the records cut into T ranges formatted side by side, written in order
		std::vector<std::thread> pool;
		const uint64_t per = (n + T - 1) / T;
		for (unsigned t = 0; t < T; t++) {
			const uint64_t a = std::min(n, t * per), b = std::min(n, (t + 1) * per);
			pool.emplace_back([&, t, a, b]() {
				std::string& out = outs[t];
				out.clear();
				for (uint64_t r = a; r < b; r++) {
					const uint64_t len = off[r + 1] - off[r];
					if (len < k) continue;
					for (uint64_t j = 0; j + k <= len; j++)
						if (print[off[r] + j]) kn::format_kmer(out, o.format, ids[r], seqCount + r, j, k, seqs.data() + off[r] + j);
				}
			});
		}
		for (auto& th : pool) th.join();
		for (unsigned t = 0; t < T; t++) fwrite(outs[t].data(), 1, outs[t].size(), stdout);
		if (o.verbose)
			for (uint64_t r = 0; r < n; r++)
				if (off[r + 1] - off[r] >= k && (seqCount + r) % 1000 == 0) fprintf(stderr, "processed %llu sequences\n", (unsigned long long)(seqCount + r));
		seqCount += n;
	}
	abg_kn_destroy(kf);
	if (o.verbose) fprintf(stderr, "processed %llu sequences\n", (unsigned long long)seqCount);
	if (fflush(stdout) != 0) return EXIT_FAILURE;
	return EXIT_SUCCESS;
}

int main(int argc, char** argv)
{
	if (argc < 2) usage_error();
	const std::string command = argv[1];
	if (command == "--help" || command == "-h") { fputs(USAGE, stdout); return EXIT_SUCCESS; }
	if (command == "--version") { puts(PROGRAM " (abyss_amd)"); return EXIT_SUCCESS; }
	if (command == "build") {
		// the type first: `-t counting' and `-t rolling-hash' keep their own parser (build_btl)
		std::string type = "konnector";
		opterr = 0;
		optind = 2;
		for (int c; (c = getopt_long(argc, argv, kn_shortopts, kn_longopts, NULL)) != -1;)
			if (c == 't') type = optarg;
		opterr = 1;
		if (type == "counting" || type == "rolling-hash") return build_btl(argc, argv);
		if (type != "konnector") {
			fprintf(stderr, PROGRAM ": unrecognized argument to `-t' (should be 'konnector', 'rolling-hash' or 'counting')\n");
			usage_error();
		}
		const KnOpts o = parse_opts(argc, argv);
		return build_konnector(argc, argv, o);
	}
	if (command == "union") return combine(argc, argv, kn::OR);
	if (command == "intersect") return combine(argc, argv, kn::AND);
	if (command == "info") return info(argc, argv);
	if (command == "compare") return compare(argc, argv);
	if (command == "kmers" || command == "getKmers") return kmers(argc, argv);
	if (command == "graph" || command == "trim") {
		fprintf(stderr, PROGRAM ": `%s' is not provided by this build (it walks a DBGBloom graph on the CPU)\n", command.c_str());
		return EXIT_FAILURE;
	}
	fprintf(stderr, PROGRAM ": unrecognized command: `%s'\n", command.c_str());
	usage_error();
}
