// de_check -- DistanceEst without a GPU, for the CPU suite: the same distanceest_core.h as abyss_amd/bin/DistanceEst over the bodies
// of abg_de.h run serially (what the kernel must equal bit for bit).
//   de_check run ARGS...          what `DistanceEst ARGS...` writes (stdout, -o file, stderr, status)
//   de_check scan JOBS OUT        the scan's arrays for a job file: c (f64), L (f64), n (u32), job after job
//   de_check dump JOBS ARGS...    reads as `run ARGS...` does and writes every contig pair that reaches the estimator as a job file,
//                                 with the pair records and, in JOBS.labels, the edge of each; it estimates nothing
// A job file, little-endian: u64 npmf, f64 minp, f64 mean, f64 pmf[npmf], u64 njobs, {i32 first, last; u32 len0, len1}[njobs],
// u64 offsets[njobs + 1], i32 values[], u32 counts[]; `dump` appends {i32 first, last; u32 len0, len1, l, rf}[njobs],
// u64 sample_offsets[njobs + 1], i32 samples[].
#include <fstream>

#include "../../abyss_amd/csrc/host/distanceest_core.h"

namespace {

template <class T> void put(FILE* f, const std::vector<T>& v) { if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f); }
template <class T> bool get(FILE* f, std::vector<T>& v, size_t n) { v.resize(n); return n == 0 || fread(v.data(), sizeof(T), n, f) == n; }

struct DumpBackend : de::SerialBackend {
	std::string path;
	std::vector<abg::DEPair> all_pairs;
	std::vector<abg::DEJob> jobs;
	std::vector<uint64_t> hoff{ 0 }, soff{ 0 };
	std::vector<int32_t> values, all_samples;
	std::vector<uint32_t> counts;
	std::vector<std::string> labels;
	bool wants_labels() const override { return true; }
	void label(const std::string& s) override { labels.push_back(s); }
	bool estimate(const std::vector<abg::DEPair>& pairs, const std::vector<int32_t>& samples, const std::vector<uint64_t>& off, int32_t* d,
	    uint32_t* n, std::string& err) override
	{
		for (size_t i = 0; i < pairs.size(); ++i) { // (nothing is estimated: what this run prints is not looked at)
			abg::DEPrepared p;
			if (const char* why = abg::de_prepare(pairs[i], samples.data() + off[i], off[i + 1] - off[i], (int)pmf.size(), mean, p)) {
				err = why;
				return false;
			}
			d[i] = 0;
			n[i] = 0;
			jobs.push_back(p.job);
			values.insert(values.end(), p.values.begin(), p.values.end());
			counts.insert(counts.end(), p.counts.begin(), p.counts.end());
			hoff.push_back(values.size());
			all_pairs.push_back(pairs[i]);
			all_samples.insert(all_samples.end(), samples.begin() + off[i], samples.begin() + off[i + 1]);
			soff.push_back(all_samples.size());
		}
		return true;
	}
	bool write() const
	{
		FILE* f = fopen(path.c_str(), "wb");
		if (!f) return false;
		const uint64_t np = pmf.size(), nj = jobs.size();
		fwrite(&np, 8, 1, f); fwrite(&minp, 8, 1, f); fwrite(&mean, 8, 1, f);
		put(f, pmf);
		fwrite(&nj, 8, 1, f);
		put(f, jobs); put(f, hoff); put(f, values); put(f, counts);
		put(f, all_pairs); put(f, soff); put(f, all_samples);
		std::ofstream l(path + ".labels");
		for (auto& s : labels) l << s << '\n';
		return fclose(f) == 0;
	}
};

int scan(const char* in, const char* out)
{
	FILE* f = fopen(in, "rb");
	if (!f) { fprintf(stderr, "de_check: cannot read %s\n", in); return 2; }
	uint64_t np = 0, nj = 0;
	double minp = 0, mean = 0;
	std::vector<double> pmf;
	std::vector<abg::DEJob> jobs;
	std::vector<uint64_t> off;
	std::vector<int32_t> values;
	std::vector<uint32_t> counts;
	bool ok = fread(&np, 8, 1, f) == 1 && fread(&minp, 8, 1, f) == 1 && fread(&mean, 8, 1, f) == 1 && get(f, pmf, np) && fread(&nj, 8, 1, f) == 1
	    && get(f, jobs, nj) && get(f, off, nj + 1);
	ok = ok && get(f, values, off[nj]) && get(f, counts, off[nj]);
	fclose(f);
	if (!ok) { fprintf(stderr, "de_check: %s is cut short\n", in); return 2; }
	std::vector<double> logp(np);
	for (uint64_t i = 0; i < np; ++i) logp[i] = log(pmf[i]);
	FILE* o = fopen(out, "wb");
	if (!o) { fprintf(stderr, "de_check: cannot write %s\n", out); return 2; }
	std::vector<double> c, like;
	std::vector<uint32_t> n;
	for (uint64_t i = 0; i < nj; ++i) {
		const size_t t = jobs[i].last < jobs[i].first ? 0 : (size_t)((int64_t)jobs[i].last - jobs[i].first + 1);
		c.assign(t, 0); like.assign(t, 0); n.assign(t, 0);
		abg::de_scan_job(jobs[i], values.data() + off[i], counts.data() + off[i], off[i + 1] - off[i], pmf.data(), logp.data(), (int)np, minp,
		    log(minp), c.data(), like.data(), n.data());
		put(o, c); put(o, like); put(o, n);
	}
	return fclose(o) == 0 ? 0 : 2;
}

} // namespace

int main(int argc, char** argv)
{
	const std::string mode = argc > 1 ? argv[1] : "";
	if (mode == "run") {
		de::SerialBackend be;
		argv[1] = argv[0];
		return de::run_main(argc - 1, argv + 1, be);
	}
	if (mode == "scan" && argc == 4) return scan(argv[2], argv[3]);
	if (mode == "dump" && argc > 3) {
		DumpBackend be;
		be.path = argv[2];
		argv[2] = argv[0];
		const int st = de::run_main(argc - 2, argv + 2, be);
		if (!be.write()) { fprintf(stderr, "de_check: cannot write %s\n", be.path.c_str()); return 2; }
		return st;
	}
	fprintf(stderr, "usage: de_check run ARGS... | scan JOBS OUT | dump JOBS ARGS...\n");
	return 2;
}
