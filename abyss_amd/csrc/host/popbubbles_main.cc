// PopBubbles -- drop-in for ABySS's PopBubbles (bin/abyss-pe:604-605): popbubbles_core.h over libabyss_amd.so.
// The HIP runtime starts when the first bubble has passed the cheap tests and its branches have to be aligned: a run with -p0, a
// graph with no such bubble, and every error that comes before that point, never opens the device.
#include "abyss_amd.h"
#include "popbubbles_core.h"

namespace {

struct GpuAligner : pb::Aligner {
	abg_pb* s = nullptr;
	~GpuAligner() override { if (s) abg_pb_destroy(s); }
	bool open(std::string& err) override
	{
		if (abg_pb_create(0, &s) == ABG_OK) return true;
		err = abg_pb_last_error(nullptr);
		return false;
	}
	// groups of two go out as pairs in one call, groups of three and more as chains in another: one launch a round
	bool align(const std::vector<std::vector<std::string>>& groups, std::vector<uint32_t>& matches, std::vector<uint32_t>& size, std::string& err) override
	{
		const size_t n = groups.size();
		matches.assign(n, 0);
		size.assign(n, 0);
		std::vector<size_t> pairs, chains;
		for (size_t i = 0; i < n; i++) (groups[i].size() == 2 ? pairs : chains).push_back(i);
		const uint8_t* cons = nullptr;
		if (!pairs.empty()) {
			std::string a, b;
			std::vector<uint64_t> aoff(1, 0), boff(1, 0), coff(pairs.size() + 1, 0);
			for (size_t i : pairs) {
				a += groups[i][0];
				b += groups[i][1];
				aoff.push_back(a.size());
				boff.push_back(b.size());
			}
			std::vector<uint32_t> m(pairs.size()), sz(pairs.size());
			std::vector<uint8_t> redone(pairs.size());
			if (abg_pb_align(s, pairs.size(), (const uint8_t*)a.data(), aoff.data(), (const uint8_t*)b.data(), boff.data(), 0, m.data(), sz.data(), redone.data(), coff.data(),
			        &cons) != ABG_OK) {
				err = abg_pb_last_error(s);
				return false;
			}
			for (size_t j = 0; j < pairs.size(); j++) { matches[pairs[j]] = m[j]; size[pairs[j]] = sz[j]; }
		}
		if (!chains.empty()) {
			std::string bytes;
			std::vector<uint64_t> first(1, 0), off(1, 0), coff(chains.size() + 1, 0);
			for (size_t i : chains) {
				for (const std::string& q : groups[i]) { bytes += q; off.push_back(bytes.size()); }
				first.push_back(off.size() - 1);
			}
			std::vector<uint32_t> m(chains.size()), sz(chains.size());
			std::vector<uint8_t> redone(chains.size());
			if (abg_pb_align_chain(s, chains.size(), first.data(), (const uint8_t*)bytes.data(), off.data(), m.data(), sz.data(), redone.data(), coff.data(), &cons) != ABG_OK) {
				err = abg_pb_last_error(s);
				return false;
			}
			for (size_t j = 0; j < chains.size(); j++) { matches[chains[j]] = m[j]; size[chains[j]] = sz[j]; }
		}
		return true;
	}
};

} // namespace

int main(int argc, char** argv)
{
	GpuAligner a;
	return pb::run_main(argc, argv, a);
}
