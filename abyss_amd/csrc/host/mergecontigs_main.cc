// MergeContigs -- drop-in for ABySS's MergeContigs (bin/abyss-pe:600-892): mergecontigs_core.h over libabyss_amd.so.
// The HIP runtime starts when the first path of two or more nodes has to be merged: a run whose paths all hold one node (or none),
// and every error that comes before that point, never opens the device.
#include "abyss_amd.h"
#include "mergecontigs_core.h"

namespace {

struct GpuMerger : mc::Merger {
	abg_mc* s = nullptr;
	~GpuMerger() override { if (s) abg_mc_destroy(s); }
	bool open(std::string& err) override
	{
		if (abg_mc_create(0, &s) == ABG_OK) return true;
		err = abg_mc_last_error(nullptr);
		return false;
	}
	bool set_contigs(const std::string& bytes, const std::vector<uint64_t>& offsets, std::string& err) override
	{
		if (abg_mc_set_contigs(s, (const uint8_t*)bytes.data(), offsets.data(), offsets.size() - 1) == ABG_OK) return true;
		err = abg_mc_last_error(s);
		return false;
	}
	bool merge(uint32_t k, const std::vector<uint64_t>& noff, const std::vector<mc::Node>& nodes, const std::vector<uint32_t>& ov, int verbose,
	    std::vector<uint64_t>& soff, const uint8_t*& seqs, std::vector<uint64_t>& acgt, std::vector<uint64_t>& loff, const char*& logs, std::string& err) override
	{
		const size_t n = noff.size() - 1;
		std::vector<uint8_t> redone(n, 0);
		soff.assign(n + 1, 0);
		loff.assign(n + 1, 0);
		acgt.assign(n, 0);
		if (abg_mc_merge(s, k, n, noff.data(), nodes.data(), ov.data(), verbose, redone.data(), soff.data(), &seqs, acgt.data(), loff.data(), &logs) == ABG_OK) return true;
		err = abg_mc_last_error(s);
		return false;
	}
};

} // namespace

int main(int argc, char** argv)
{
	GpuMerger m;
	return mc::run_main(argc, argv, m);
}
