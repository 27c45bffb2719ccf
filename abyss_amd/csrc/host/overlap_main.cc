// Overlap -- drop-in for ABySS's Overlap (bin/abyss-pe:658-659): overlap_core.h over libabyss_amd.so.
// The HIP runtime starts when the first pair has to be searched: a run in which no estimate reaches findOverlap, and every error
// that comes before that point, never opens the device.
#include "abyss_amd.h"
#include "overlap_core.h"

namespace {

struct GpuSearcher : ov::Searcher {
	abg_ov* o = nullptr;
	~GpuSearcher() override { if (o) abg_ov_destroy(o); }
	bool open(std::string& err) override
	{
		if (abg_ov_create(0, &o) == ABG_OK) return true;
		err = abg_ov_last_error(nullptr);
		return false;
	}
	bool set_contigs(const std::string& bytes, const std::vector<uint64_t>& offsets, std::string& err) override
	{
		if (abg_ov_set_contigs(o, (const uint8_t*)bytes.data(), offsets.data(), offsets.size() - 1) == ABG_OK) return true;
		err = abg_ov_last_error(o);
		return false;
	}
	bool find(const std::vector<std::pair<ov::V, ov::V>>& pairs, bool all, std::vector<uint32_t>& top, std::vector<uint32_t>& ntop,
	    std::vector<uint64_t>& all_offsets, std::vector<uint32_t>& lengths, std::string& err) override
	{
		static_assert(sizeof(std::pair<ov::V, ov::V>) == sizeof(abg_ov_pair), "ABI struct");
		const abg_ov_pair* p = (const abg_ov_pair*)pairs.data();
		int rc;
		if (all) {
			all_offsets.assign(pairs.size() + 1, 0);
			const uint32_t* l = nullptr;
			rc = abg_ov_find(o, p, pairs.size(), ABG_OV_ALL, nullptr, nullptr, all_offsets.data(), &l);
			if (rc == ABG_OK) lengths.assign(l, l + all_offsets[pairs.size()]);
		} else {
			top.assign(3 * pairs.size(), 0);
			ntop.assign(pairs.size(), 0);
			rc = abg_ov_find(o, p, pairs.size(), ABG_OV_TOP, top.data(), ntop.data(), nullptr, nullptr);
		}
		if (rc == ABG_OK) return true;
		err = abg_ov_last_error(o);
		return false;
	}
};

} // namespace

int main(int argc, char** argv)
{
	GpuSearcher s;
	return ov::run_main(argc, argv, s);
}
