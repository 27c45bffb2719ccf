// abyss-mergepairs -- drop-in for ABySS's abyss-mergepairs (Align/mergepairs.cc): mergepairs_core.h over libabyss_amd.so.
// The HIP runtime starts when the first batch of pairs is ready to be aligned: empty inputs, every option error and a file that
// cannot be opened never open the device.  At -vvv the alignments are printed, which needs the whole matrix: the host's, pair by
// pair, as the reference runs it.
#include "abyss_amd.h"
#include "mergepairs_core.h"

namespace {

struct GpuAligner : mp::Aligner {
	abg_mp* s = nullptr;
	~GpuAligner() override { close(); }
	void close() override
	{
		if (s) abg_mp_destroy(s);
		s = nullptr;
	}
	bool open(std::string& err) override
	{
		if (abg_mp_create(0, &s) == ABG_OK) return true;
		err = abg_mp_last_error(nullptr);
		return false;
	}
	// (the kernel complements read 2 itself)
	bool align(const std::vector<mp::Record>& r1, const std::vector<mp::Record>& r2, const std::vector<std::string>&, size_t n, unsigned min_matches, float identity,
	    std::vector<abg::MPRecord>& out, std::string& err) override
	{
		std::string a, b;
		std::vector<uint64_t> aoff(1, 0), boff(1, 0);
		for (size_t i = 0; i < n; i++) {
			a += r1[i].seq;
			b += r2[i].seq;
			aoff.push_back(a.size());
			boff.push_back(b.size());
		}
		out.resize(n);
		static_assert(sizeof(abg_mp_record) == sizeof(abg::MPRecord), "abg_mp_record is MPRecord");
		if (abg_mp_align(s, n, (const uint8_t*)a.data(), aoff.data(), (const uint8_t*)b.data(), boff.data(), min_matches, identity, (abg_mp_record*)out.data()) != ABG_OK) {
			err = abg_mp_last_error(s);
			return false;
		}
		return true;
	}
};

} // namespace

int main(int argc, char** argv)
{
	GpuAligner a;
	return mp::run_main(argc, argv, a);
}
