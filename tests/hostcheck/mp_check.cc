// mp_check -- abyss-mergepairs without a GPU, for the CPU suite: the same mergepairs_core.h as abyss_amd/bin/abyss-mergepairs over the
// serial body of abg_mp.h (what the kernel must equal, and what the product runs for a pair the kernel does not take).
//   mp_check run ARGS...   what `abyss-mergepairs ARGS...` writes (stdout, stderr, status, the three files).  Where the environment's
//                          MP_CHECK_COUNTS names a file it gets a line "pairs order_dependent break_taken break_not_taken" at the end.
//   mp_check align M P     stdin: a line a pair, read 1 and read 2 as the files hold them ("-" for an empty one); stdout: a line a
//                          pair, the ten fields of its record at -m M -p P, "spill" printed as 0
//   mp_check table         the 256 x 256 match table, a line a first byte, '1' where isMatch holds
//   mp_check identity P L  min_identity[1 .. L] at -p P, blank-separated
#include "../../abyss_amd/csrc/abg_mp.h"
#include "../../abyss_amd/csrc/host/mergepairs_core.h"

namespace {

struct SerialAligner : mp::Aligner {
	uint64_t pairs = 0;
	bool open(std::string&) override { return true; }
	bool align(const std::vector<mp::Record>& r1, const std::vector<mp::Record>&, const std::vector<std::string>& rc2, size_t n, unsigned min_matches, float identity, std::vector<abg::MPRecord>& out,
	    std::string&) override
	{
		uint32_t longest = 0;
		for (size_t i = 0; i < n; i++) longest = std::max<uint32_t>(longest, (uint32_t)(r1[i].seq.size() + rc2[i].size()));
		const std::vector<uint32_t> min_identity = abg::mp_identity_table(identity, longest);
		out.resize(n);
		for (size_t i = 0; i < n; i++) abg::mp_align_host(r1[i].seq, rc2[i], min_matches, min_identity.data(), out[i]);
		pairs += n;
		return true;
	}
};

void write_counts(const SerialAligner& a)
{
	if (const char* path = getenv("MP_CHECK_COUNTS"))
		if (FILE* f = fopen(path, "w")) {
			fprintf(f, "%llu %llu %llu %llu\n", (unsigned long long)a.pairs, (unsigned long long)a.order_dependent, (unsigned long long)a.break_taken,
			    (unsigned long long)a.break_not_taken);
			fclose(f);
		}
}

} // namespace

int main(int argc, char** argv)
{
	const std::string mode = argc > 1 ? argv[1] : "";
	if (mode == "run") {
		SerialAligner a;
		argv[1] = argv[0];
		const int rc = mp::run_main(argc - 1, argv + 1, a);
		write_counts(a);
		return rc;
	}
	if (mode == "align" && argc == 4) {
		const unsigned min_matches = (unsigned)strtoul(argv[2], nullptr, 10);
		const float identity = strtof(argv[3], nullptr);
		std::string line;
		while (std::getline(std::cin, line)) {
			std::istringstream ss(line);
			std::string a, b;
			if (!(ss >> a >> b)) { fprintf(stderr, "mp_check: a line holds two reads\n"); return 2; }
			if (a == "-") a.clear();
			if (b == "-") b.clear();
			for (char c : b)
				if (!abg::ov_complement((uint8_t)c)) { fprintf(stderr, "mp_check: a byte with no complement\n"); return 2; }
			const std::string rc = abg::mp_reverse_complement(b);
			const std::vector<uint32_t> min_identity = abg::mp_identity_table(identity, (uint32_t)(a.size() + b.size()));
			abg::MPRecord r;
			abg::mp_align_host(a, rc, min_matches, min_identity.data(), r);
			printf("%u %u %u %u %u %u %u %u %u 0\n", r.n_aligned, r.n_matches, r.n_identity, r.n_gapless, r.t_pos, r.h_pos, r.length, r.matches, r.flags);
		}
		return 0;
	}
	if (mode == "table") {
		const std::vector<uint32_t> t = abg::mp_match_table();
		for (int a = 0; a < 256; a++) {
			for (int b = 0; b < 256; b++) putchar(abg::mp_table_match(t.data(), (uint8_t)a, (uint8_t)b) ? '1' : '0');
			putchar('\n');
		}
		return 0;
	}
	if (mode == "identity" && argc == 4) {
		const std::vector<uint32_t> t = abg::mp_identity_table(strtof(argv[2], nullptr), (uint32_t)strtoul(argv[3], nullptr, 10));
		for (size_t L = 1; L < t.size(); L++) printf("%u%c", t[L], L + 1 < t.size() ? ' ' : '\n');
		return 0;
	}
	fprintf(stderr, "usage: mp_check run ARGS... | align M P | table | identity P L\n");
	return 2;
}
