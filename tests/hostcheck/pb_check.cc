// pb_check -- PopBubbles without a GPU, for the CPU suite: the same popbubbles_core.h as abyss_amd/bin/PopBubbles over the serial
// text of abg_pb.h (what the kernels must equal, and what the product runs for a pair that fits no arena).
//   pb_check run ARGS...   what `PopBubbles ARGS...` writes (stdout, stderr, status, the -g file); the number of groups of branches it
//                          has had aligned so far goes to the file the environment's PB_CHECK_GROUPS names, at every batch
//   pb_check align         stdin: a line a group, its sequences separated by blanks ("-" for an empty one); stdout: matches, size and
//                          consensus ("-" when empty) of align(seqs)
//   pb_check codes         pb_code_match against pb_score on every pair of codes of either case; exits 1 where they differ
#include "../../abyss_amd/csrc/abg_pb.h"
#include "../../abyss_amd/csrc/host/popbubbles_core.h"

namespace {

struct SerialAligner : pb::Aligner {
	uint64_t groups_seen = 0;
	bool open(std::string&) override { return true; }
	bool align(const std::vector<std::vector<std::string>>& groups, std::vector<uint32_t>& matches, std::vector<uint32_t>& size, std::string& err) override
	{
		matches.assign(groups.size(), 0);
		size.assign(groups.size(), 0);
		groups_seen += groups.size();
		if (const char* path = getenv("PB_CHECK_GROUPS")) { // for the tests: does this run need the device at all?
			if (FILE* f = fopen(path, "w")) { fprintf(f, "%llu\n", (unsigned long long)groups_seen); fclose(f); }
		}
		for (size_t i = 0; i < groups.size(); i++) {
			for (const std::string& s : groups[i])
				for (char c : s)
					if (!abg::pb_code((uint8_t)c)) { err = "a branch holds a byte that is no nucleotide or IUPAC code"; return false; }
			abg::pb_align_group_host(groups[i], matches[i], size[i], nullptr);
		}
		return true;
	}
};

} // namespace

int main(int argc, char** argv)
{
	const std::string mode = argc > 1 ? argv[1] : "";
	if (mode == "run") {
		SerialAligner a;
		argv[1] = argv[0];
		return pb::run_main(argc - 1, argv + 1, a);
	}
	if (mode == "align") {
		std::string line;
		while (std::getline(std::cin, line)) {
			std::istringstream ss(line);
			std::vector<std::string> seqs;
			for (std::string s; ss >> s;) seqs.push_back(s == "-" ? "" : s);
			if (seqs.size() < 2) { fprintf(stderr, "pb_check: a group has two sequences or more\n"); return 2; }
			uint32_t m = 0, n = 0;
			std::string cons;
			abg::pb_align_group_host(seqs, m, n, &cons);
			printf("%u %u %s\n", m, n, cons.empty() ? "-" : cons.c_str());
		}
		return 0;
	}
	if (mode == "codes") {
		const std::string codes = "ACGTMRWSYKVHDBNacgtmrwsykvhdbn";
		int bad = 0;
		for (char a : codes)
			for (char b : codes) {
				uint8_t c;
				const bool want = abg::pb_score((uint8_t)a, (uint8_t)b, c) == abg::PB_MATCH;
				if (abg::pb_code_match(abg::pb_code((uint8_t)a), abg::pb_code((uint8_t)b)) != want) { printf("%c %c: pb_score says %d\n", a, b, want); bad = 1; }
			}
		for (int c = 0; c < 256; c++)
			if ((abg::pb_code((uint8_t)c) != 0) != (c != 0 && codes.find((char)c) != std::string::npos)) { printf("byte %d\n", c); bad = 1; }
		return bad;
	}
	fprintf(stderr, "usage: pb_check run ARGS... | align | codes\n");
	return 2;
}
