// DistanceEst -- drop-in for ABySS's DistanceEst (bin/abyss-pe:632-644, 722-734): distanceest_core.h over libabyss_amd.so.
// --mean and --median never reach the backend, so they never start the HIP runtime; --mle opens the device when the first batch of
// contig pairs is ready, after the option and input checks.
#include "abyss_amd.h"
#include "distanceest_core.h"

namespace {

struct GpuBackend : de::Backend {
	abg_de* d = nullptr;
	~GpuBackend() override { if (d) abg_de_destroy(d); }
	bool open(std::string& err) override
	{
		if (abg_de_create(0, &d) == ABG_OK) return true;
		err = abg_de_last_error(nullptr);
		return false;
	}
	bool set_pmf(const std::vector<double>& pmf, double minp, double mean, std::string& err) override
	{
		if (abg_de_set_pmf(d, pmf.data(), pmf.size(), minp, mean) == ABG_OK) return true;
		err = abg_de_last_error(d);
		return false;
	}
	bool estimate(const std::vector<abg::DEPair>& pairs, const std::vector<int32_t>& samples, const std::vector<uint64_t>& offsets,
	    int32_t* distance, uint32_t* num_pairs, std::string& err) override
	{
		static_assert(sizeof(abg::DEPair) == sizeof(abg_de_pair), "ABI struct");
		if (abg_de_estimate(d, (const abg_de_pair*)pairs.data(), pairs.size(), samples.data(), offsets.data(), distance, num_pairs) == ABG_OK)
			return true;
		err = abg_de_last_error(d);
		return false;
	}
};

} // namespace

int main(int argc, char** argv)
{
	GpuBackend be;
	return de::run_main(argc, argv, be);
}
