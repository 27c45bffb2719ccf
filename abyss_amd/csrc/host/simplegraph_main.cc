// SimpleGraph -- drop-in for ABySS's SimpleGraph (bin/abyss-pe:663-664): simplegraph_core.h over libabyss_amd.so.
// The HIP runtime starts when the first search has to be done: a run in which no contig end has estimates left, and every error
// that comes before that point, never opens the device.
#include "abyss_amd.h"
#include "simplegraph_core.h"

namespace {

struct GpuSearcher : sg::Searcher {
	abg_sg* s = nullptr;
	~GpuSearcher() override { if (s) abg_sg_destroy(s); }
	bool open(std::string& err) override
	{
		if (abg_sg_create(0, &s) == ABG_OK) return true;
		err = abg_sg_last_error(nullptr);
		return false;
	}
	bool set_graph(const std::vector<uint64_t>& eoff, const std::vector<uint32_t>& lengths, const std::vector<uint32_t>& targets,
	    const std::vector<int32_t>& distances, std::string& err) override
	{
		if (abg_sg_set_graph(s, lengths.size(), eoff.data(), lengths.data(), targets.data(), distances.data()) == ABG_OK) return true;
		err = abg_sg_last_error(s);
		return false;
	}
	bool search(const std::vector<uint32_t>& origins, const std::vector<uint64_t>& coff, const std::vector<uint32_t>& cv, const std::vector<int32_t>& cb,
	    uint32_t max_cost, uint32_t max_paths, std::vector<uint32_t>& visited, std::vector<uint64_t>& index, std::vector<uint64_t>& poff,
	    std::vector<uint32_t>& nodes, std::string& err) override
	{
		const size_t n = origins.size();
		visited.assign(n, 0);
		index.assign(n + 1, 0);
		std::vector<uint8_t> redone(n, 0);
		const uint64_t* po = nullptr;
		const uint32_t* pn = nullptr;
		if (abg_sg_search(s, n, origins.data(), coff.data(), cv.data(), cb.data(), max_cost, max_paths, visited.data(), redone.data(), index.data(), &po, &pn)
		    != ABG_OK) {
			err = abg_sg_last_error(s);
			return false;
		}
		poff.assign(po, po + index[n] + 1);
		nodes.assign(pn, pn + poff[index[n]]);
		return true;
	}
};

} // namespace

int main(int argc, char** argv)
{
	GpuSearcher s;
	return sg::run_main(argc, argv, s);
}
