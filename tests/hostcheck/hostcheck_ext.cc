// libhostcheck.so is built from this file: hostcheck.cc as it stands, and after it the entry points that came later.
// The next entry point goes into this file too, not into a third one.
#include "hostcheck.cc"

extern "C" {

// the parallel commit's counters that abg_stats got after hc_get_stats was written:
// out[0] commit_rounds_incremental, out[1] commit_dirty_records, out[2] commit_first_chunk_decided
void hc_get_commit_stats(void* h, uint64_t* out)
{
	auto s = S(h)->eng->stats();
	out[0] = s.commit_rounds_incremental; out[1] = s.commit_dirty_records; out[2] = s.commit_first_chunk_decided;
}

} // extern "C"
