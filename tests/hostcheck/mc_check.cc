// mc_check -- MergeContigs without a GPU, for the CPU suite: the same mergecontigs_core.h as abyss_amd/bin/MergeContigs over the
// serial text of abg_mc.h (what the kernels must equal, and what the product runs for the paths they flag).
//   mc_check run ARGS...        what `MergeContigs ARGS...` writes (the -o and -g files, stdout, stderr, status)
#include "../../abyss_amd/csrc/abg_mc.h"
#include "../../abyss_amd/csrc/host/mergecontigs_core.h"

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

} // namespace

int main(int argc, char** argv)
{
	const std::string mode = argc > 1 ? argv[1] : "";
	if (mode == "run") {
		SerialMerger m;
		argv[1] = argv[0];
		return mc::run_main(argc - 1, argv + 1, m);
	}
	fprintf(stderr, "usage: mc_check run ARGS...\n");
	return 2;
}
