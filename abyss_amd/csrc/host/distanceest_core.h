// distanceest_core.h -- everything of DistanceEst but the scan over theta: options, the fragment-size histogram and its PMF, the
// SAM reader, the grouping of pairs and the three output formats.  abyss_amd/bin/DistanceEst runs it over libabyss_amd.so
// (abg_de_estimate); tests/hostcheck/de_check runs it over the serial bodies of abg_de.h.
//
// Reference behaviour restated here (ABySS 2.3.10, paths relative to the repo):
//   DistanceEst/DistanceEst.cpp:114-152  the option table; :433-515 its messages and statuses
//   DistanceEst/DistanceEst.cpp:566-626  histogram -> orientation -> negate / eraseNegative / removeNoise / removeOutliers /
//                                        trimFraction(0.0001) -> PMF; the -v lines
//   Common/Histogram.h, Histogram.cpp    percentile (a float product), mean, sd, trimFraction, bin and barplot
//   Common/PMF.h                         p[i] = n / count or 1 / count where n == 0; count is the 32-bit size
//   Common/SAM.h:335-372, 382-407        a record (the /1 /2 suffix sets the paired flag, a span under -l the unmapped flag); @SQ
//   Common/SAM.h:147-154, 307-310        targetAtQueryStart, mateTargetAtQueryStart
//   DistanceEst/DistanceEst.cpp:400-431  the record filter; a target's records are consecutive; the sortedness check
//   DistanceEst/DistanceEst.cpp:338-377  two senses, mates keyed by ContigNode (2 * id + sense), in the map's order
//   DistanceEst/DistanceEst.cpp:219-295  fragments, sort, unique, the duplicate statistics, the `ma` reduction
//   DistanceEst/DistanceEst.cpp:297-335, Common/Estimate.h:47-69  dist, dot and GFA2 lines; GFA2 prints one of two complementary edges
//
// Output is in input order whatever -j is (the reference's -j1 order).  Input may be a pipe: it is read in large blocks cut at
// line ends, parsed on the -j threads, and only (target, mate, strands, the two extrapolated positions) are kept per record.
#pragma once
#include <getopt.h>

#include <algorithm>
#include <cerrno>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iomanip>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../abg_de.h"

namespace de {

enum { FMT_DIST, FMT_DOT, FMT_GFA2 };
enum { M_MLE, M_MEAN, M_MEDIAN };

struct Options {
	int format = FMT_DIST, method = M_MLE, rf = -1, verbose = 0, threads = 1;
	int min_dist = INT_MIN, max_dist = INT_MAX;
	unsigned k = 0, min_align = 1, seed_len = 0, npairs = 0, min_mapq = 10;
	std::string out, hist, sam = "-";
};

// the estimator behind --mle: the GPU library in the binary, the serial bodies in de_check
struct Backend {
	virtual ~Backend() {}
	virtual bool open(std::string& err) = 0;
	virtual bool set_pmf(const std::vector<double>& pmf, double minp, double mean, std::string& err) = 0;
	virtual bool estimate(const std::vector<abg::DEPair>& pairs, const std::vector<int32_t>& samples, const std::vector<uint64_t>& offsets,
	    int32_t* distance, uint32_t* num_pairs, std::string& err) = 0;
	// the edge ("a+ b-") of the pair that the next estimate() will hold at this index; only de_check's job dump listens
	virtual bool wants_labels() const { return false; }
	virtual void label(const std::string&) {}
};

static const char USAGE[] =
    "Usage: DistanceEst -k<kmer> -s<seed-length> -n<npairs> [OPTION]... HIST [PAIR]\n"
    "Estimate the distances between contigs from read pairs aligned to two contigs.\n"
    "HIST is the fragment-size histogram, PAIR the alignments (SAM sorted by target; standard input by default).\n"
    "\n"
    "      --mind=N, --maxd=N   the least and the greatest distance [-(k-1), the greatest fragment]\n"
    "      --fr, --rf           force the orientation of the library\n"
    "  -k, --kmer=N             --mind defaults to -(k-1)\n"
    "  -l, --min-align=N        the aligner's minimal alignment [1]\n"
    "  -n, --npairs=N           the fewest pairs an estimate needs\n"
    "  -s, --seed-length=N      the shortest contig to estimate from\n"
    "  -q, --min-mapq=N         the least mapping quality [10]\n"
    "  -o, --out=FILE           write to FILE\n"
    "      --mle, --median, --mean      the estimator [--mle: maximum likelihood, on the GPU]\n"
    "      --dist, --dot, --gv, --gfa, --gfa2   the output format [--dist]\n"
    "  -j, --threads=N          host threads [1], at most 16; the output is in input order whatever N\n"
    "  -v, --verbose            say more\n"
    "      --help, --version\n"
    "      --db, --library, --strain, --species   accepted and ignored\n";

struct Hist {
	std::map<int, size_t> m;
	void insert(int v, size_t c = 1) { m[v] += c; }
	bool empty() const { return m.empty(); }
	size_t count(int v) const { auto it = m.find(v); return it == m.end() ? 0 : it->second; }
	size_t count(int lo, int hi) const
	{
		size_t n = 0;
		for (auto it = m.lower_bound(lo), last = m.upper_bound(hi); it != last; ++it) n += it->second;
		return n;
	}
	int minimum() const { return empty() ? 0 : m.begin()->first; }
	int maximum() const { return empty() ? 0 : m.rbegin()->first; }
	size_t size() const { size_t n = 0; for (auto& e : m) n += e.second; return n; }
	double mean() const
	{
		unsigned long long n = 0, total = 0;
		for (auto& e : m) { n += e.second; total += (unsigned long long)e.first * e.second; }
		return (double)total / n;
	}
	double sd() const
	{
		unsigned long long n = 0, total = 0, squares = 0;
		for (auto& e : m) {
			n += e.second;
			total += (unsigned long long)e.first * e.second;
			squares += (unsigned long long)e.first * e.first * e.second;
		}
		return sqrt((squares - (double)total * total / n) / n);
	}
	int percentile(float p) const
	{
		const size_t x = (size_t)ceil(p * size()); // (a float product, as the reference's)
		size_t n = 0;
		for (auto& e : m) { n += e.second; if (n >= x) return e.first; }
		return maximum();
	}
	int median() const { return percentile(0.5); }
	void erase_negative() { for (auto it = m.begin(); it != m.end();) it = it->first < 0 ? m.erase(it) : std::next(it); }
	void remove_noise() // a value with neither neighbour present
	{
		for (auto it = m.begin(); it != m.end();)
			it = m.count(it->first - 1) == 0 && m.count(it->first + 1) == 0 && m.size() > 1 ? m.erase(it) : std::next(it);
	}
	void remove_outliers() // outside [Q1 - 20 IQR, Q3 + 20 IQR]
	{
		const int q1 = percentile(0.25), q3 = percentile(0.75), l = q1 - 20 * (q3 - q1), u = q3 + 20 * (q3 - q1);
		for (auto it = m.begin(); it != m.end();) it = it->first < l || it->first > u ? m.erase(it) : std::next(it);
	}
	Hist negate() const { Hist h; for (auto& e : m) h.m.insert({ -e.first, e.second }); return h; }
	Hist trim_fraction(double fraction) const
	{
		const double low = fraction / 2, high = 1.0f - fraction / 2;
		const size_t n = size();
		double cumulative = 0;
		Hist h;
		for (auto& e : m) {
			const double t = cumulative + (double)e.second / n;
			if (t > low && cumulative < high) h.insert(e.first, e.second);
			cumulative = t;
		}
		return h;
	}
	std::string barplot() const
	{
		static const char* bars[10] = { " ", "_", "\342\226\201", "\342\226\202", "\342\226\203", "\342\226\204", "\342\226\205", "\342\226\206",
			"\342\226\207", "\342\226\210" };
		const char* columns = getenv("COLUMNS");
		const unsigned nbins = columns == NULL ? 80 : strtoul(columns, NULL, 0);
		std::vector<unsigned long long> bins;
		if (empty()) return "";
		const int per = (int)ceilf((float)(maximum() - minimum()) / nbins);
		int next = minimum() + per;
		unsigned long long count = 0;
		for (auto& e : m) {
			if (e.first >= next) { bins.push_back(count); count = 0; next += per; }
			count += e.second;
		}
		if (count > 0) bins.push_back(count);
		const unsigned long long max = 1 + *std::max_element(bins.begin(), bins.end());
		std::string s;
		for (unsigned long long b : bins) s += bars[10 * b / max];
		while (!s.empty() && s.back() == ' ') s.pop_back();
		return s;
	}
};

struct Pmf {
	std::vector<double> p;
	double mean = 0, sd = 0, minp = 0;
	int median = 0;
	explicit Pmf(const Hist& h) : p(h.maximum() + 1), mean(h.mean()), sd(h.sd()), median(h.median())
	{
		const unsigned count = h.size();
		minp = (double)1 / count;
		for (size_t i = 0; i < p.size(); i++) {
			const unsigned n = h.count((int)i);
			p[i] = n > 0 ? (double)n / count : minp;
		}
	}
	double at(int x) const { return x >= 0 && (size_t)x < p.size() ? p[x] : minp; }
	int max_value() const { return (int)p.size() - 1; }
};

// what is kept of one SAM record that passed the filter
struct Rec { uint32_t r, m; int32_t a0, a1; uint8_t rev, mrev; };

struct Entry { // one writeEstimate that got past the first pair count
	uint32_t id0, id1, len1, pairs_in;
	int32_t d = INT_MIN;
	uint32_t n = 0;
	int64_t job = -1;
	std::string warn; // the -v lines of estimateDistance, which the reference prints before it estimates this pair
};
struct GroupOut { uint32_t r; std::vector<Entry> e[2]; };

struct Die { int status; };

struct Run {
	Options opt;
	Backend& be;
	std::ostream& err;
	FILE* out = stdout;
	std::vector<std::string> names;
	std::vector<unsigned> lens;
	std::unordered_map<std::string, uint32_t> index;
	unsigned rec_ma = 1;
	unsigned long long total_frags = 0, dup_frags = 0; // 32-bit in the reference; printed as such
	std::vector<GroupOut> groups;
	std::vector<abg::DEPair> jobs;
	std::vector<int32_t> samples;
	std::vector<uint64_t> offsets{ 0 };
	uint64_t pending_thetas = 0;
	bool be_open = false;
	const Pmf* pmf = nullptr;
	bool no_pmf = false; // the cleaned histogram is empty: see run_main

	Run(Backend& be, std::ostream& err) : be(be), err(err) {}

	[[noreturn]] void die(const std::string& msg)
	{
		fflush(out);
		err << msg;
		err.flush();
		throw Die{ 1 };
	}

	std::string vname(uint32_t node) const { return names[node / 2] + (node & 1 ? '-' : '+'); }

	void count_agreeing(const std::map<int, unsigned>& h, int d, uint32_t& n) const
	{
		n = 0;
		for (auto& e : h)
			if (pmf->at(e.first + d) > pmf->minp) n += e.second;
	}

	void process_group(const std::vector<Rec>& recs)
	{
		const uint32_t r = recs.front().r;
		const unsigned len0 = lens[r];
		if (len0 < opt.seed_len) return;
		GroupOut g;
		g.r = r;
		std::map<uint32_t, std::vector<const Rec*>> by_mate[2];
		for (const Rec& x : recs) by_mate[x.rev][2 * x.m + (x.rev == x.mrev)].push_back(&x);
		for (int sense0 = 0; sense0 <= 1; sense0++) {
			for (auto& kv : by_mate[sense0 ^ opt.rf]) {
				const std::vector<const Rec*>& pairs = kv.second;
				if (pairs.size() < opt.npairs) continue;
				Entry e;
				e.id0 = 2 * r + sense0;
				e.id1 = kv.first;
				e.len1 = lens[kv.first / 2];
				e.pairs_in = (uint32_t)pairs.size();
				const unsigned len1 = e.len1;
				std::vector<std::pair<int, int>> frags;
				frags.reserve(pairs.size());
				for (const Rec* x : pairs) {
					int a0 = x->a0, a1 = x->a1;
					if (x->rev) a0 = len0 - a0;
					if (!x->mrev) a1 = len1 - a1;
					frags.push_back(opt.rf ? std::make_pair(a1, (int)(len1 + a0)) : std::make_pair(a0, (int)(len0 + a1)));
				}
				const size_t orig = frags.size();
				std::sort(frags.begin(), frags.end());
				frags.erase(std::unique(frags.begin(), frags.end()), frags.end());
				e.n = (uint32_t)frags.size();
				total_frags += orig;
				dup_frags += orig - frags.size();
				if (e.n >= opt.npairs && no_pmf) {
					e.d = 0;
					e.n = 0;
				} else if (e.n >= opt.npairs) {
					std::vector<int32_t> sizes;
					sizes.reserve(frags.size());
					unsigned ma = opt.min_align;
					for (auto& f : frags) {
						const int x = f.second - f.first;
						if (!opt.rf && opt.method == M_MLE && x <= 2 * int(ma - 1)) {
							const unsigned align = x / 2;
							if (opt.verbose > 0)
								e.warn += "DistanceEst: warning: The observed fragment of size " + std::to_string(x) + " bp is shorter than 2*l (l="
								    + std::to_string(opt.min_align) + ").\n";
							ma = std::min(ma, align);
						}
						sizes.push_back(x);
					}
					rec_ma = std::min(rec_ma, ma);
					if (opt.method == M_MLE) {
						e.job = (int64_t)jobs.size();
						if (be.wants_labels()) be.label(vname(e.id0) + ' ' + vname(e.id1 ^ (e.id0 & 1)));
						jobs.push_back(abg::DEPair{ opt.min_dist, opt.max_dist, len0, len1, ma, (uint32_t)opt.rf });
						samples.insert(samples.end(), sizes.begin(), sizes.end());
						offsets.push_back(samples.size());
						pending_thetas += (uint64_t)((int64_t)opt.max_dist - opt.min_dist) + abg::de_filter_size(pmf->mean) + 2;
					} else {
						std::map<int, unsigned> h;
						for (int x : sizes) h[x]++;
						if (opt.method == M_MEAN) {
							unsigned long long cnt = 0, total = 0;
							for (auto& s : h) { cnt += s.second; total += (unsigned long long)s.first * s.second; }
							e.d = (int)round(pmf->mean - (double)total / cnt);
						} else {
							const size_t x = (size_t)ceil(0.5f * sizes.size());
							size_t cnt = 0;
							int med = h.rbegin()->first;
							for (auto& s : h) { cnt += s.second; if (cnt >= x) { med = s.first; break; } }
							e.d = (int)round(pmf->median - med);
						}
						count_agreeing(h, e.d, e.n);
					}
				}
				g.e[sense0].push_back(e);
			}
		}
		groups.push_back(std::move(g));
		if (pending_thetas >= (1ull << 23) || jobs.size() >= 65536) flush();
	}

	void write_entry(std::string& line, const Entry& e)
	{
		char buf[64];
		if (e.n >= opt.npairs) {
			const float sd = pmf->sd / sqrt(e.n);
			const uint32_t e1 = e.id1 ^ (e.id0 & 1); // the mate as seen from the target's sense
			if (opt.format == FMT_DOT) {
				snprintf(buf, sizeof buf, "d=%d e=%.1f n=%u", e.d, sd, e.n);
				line += '"' + vname(e.id0) + "\" -> \"" + vname(e1) + "\" [" + buf + "]\n";
			} else if (opt.format == FMT_GFA2) {
				if (e.len1 < opt.seed_len || e.id0 <= e1) { // one of the two complementary edges
					snprintf(buf, sizeof buf, "\t%d\t%d\tFC:i:%u\n", e.d, (int)ceilf(sd), e.n);
					line += "G\t*\t" + vname(e.id0) + '\t' + vname(e1) + buf;
				}
			} else {
				snprintf(buf, sizeof buf, ",%d,%u,%.1f", e.d, e.n, sd);
				line += ' ' + vname(e.id1) + buf;
			}
		} else if (opt.verbose > 1) {
			const uint32_t e1 = e.id1 ^ (e.id0 & 1);
			err << "warning: \"" << vname(e.id0) << "\" -> \"" << vname(e1) << "\" [d=" << e.d << "] " << e.n << " of " << e.pairs_in
			    << " pairs fit the expected distribution\n";
		}
	}

	// estimates what is pending and writes every group read so far, in input order
	void flush()
	{
		std::vector<int32_t> d(jobs.size());
		std::vector<uint32_t> n(jobs.size());
		if (!jobs.empty()) {
			std::string why;
			if (!be_open) {
				if (!be.open(why) || !be.set_pmf(pmf->p, pmf->minp, pmf->mean, why)) die("DistanceEst: error: " + why + "\n");
				be_open = true;
			}
			if (!be.estimate(jobs, samples, offsets, d.data(), n.data(), why)) die("DistanceEst: error: " + why + "\n");
		}
		std::string text;
		for (GroupOut& g : groups) {
			if (opt.format == FMT_DIST) text += names[g.r];
			for (int s = 0; s <= 1; s++) {
				if (opt.format == FMT_DIST && s) text += " ;";
				for (Entry& e : g.e[s]) {
					if (e.job >= 0) { e.d = d[e.job]; e.n = n[e.job]; }
					err << e.warn;
					write_entry(text, e);
				}
			}
			if (opt.format == FMT_DIST) text += '\n';
		}
		fwrite(text.data(), 1, text.size(), out);
		groups.clear();
		jobs.clear();
		samples.clear();
		offsets.assign(1, 0);
		pending_thetas = 0;
	}
};

// ---- the SAM reader

inline bool parse_int(const char* b, const char* e, long long& v)
{
	if (b == e) return false;
	char* end;
	char tmp[32];
	const size_t n = (size_t)(e - b);
	if (n >= sizeof tmp) return false;
	memcpy(tmp, b, n);
	tmp[n] = 0;
	v = strtoll(tmp, &end, 10);
	return end != tmp; // (trailing text after the number is what `in >> int` leaves for the next field; not seen in SAM)
}

struct Cigar { unsigned qlen = 0, qstart = 0, qspan = 0, tspan = 0; bool ok = true; };
inline Cigar parse_cigar(const char* b, const char* e)
{
	Cigar c;
	if (e - b == 1 && *b == '*') return c;
	bool first = true;
	while (b < e) {
		unsigned len = 0;
		if (*b < '0' || *b > '9') break;
		while (b < e && *b >= '0' && *b <= '9') len = len * 10 + (unsigned)(*b++ - '0');
		if (b == e) break;
		switch (*b++) {
		case 'H': case 'S': if (first) c.qstart = len; c.qlen += len; break;
		case 'M': case 'X': case '=': c.qlen += len; c.qspan += len; c.tspan += len; break;
		case 'I': c.qlen += len; c.qspan += len; break;
		case 'D': case 'N': case 'P': c.tspan += len; break;
		default: c.ok = false; return c;
		}
		first = false;
	}
	return c;
}

struct ParseOut { std::vector<Rec> recs; std::string error; };

// the records of [b, e): whole lines
inline void parse_lines(const Run& run, const char* b, const char* e, ParseOut& out)
{
	const Options& opt = run.opt;
	std::string last_name, name;
	uint32_t last_index = 0;
	auto lookup = [&](const char* s, const char* t, uint32_t& idx) {
		if (!last_name.empty() && (size_t)(t - s) == last_name.size() && !memcmp(s, last_name.data(), last_name.size())) { idx = last_index; return true; }
		name.assign(s, t);
		auto it = run.index.find(name);
		if (it == run.index.end()) return false;
		last_name = name;
		idx = last_index = it->second;
		return true;
	};
	while (b < e && out.error.empty()) {
		const char* nl = (const char*)memchr(b, '\n', (size_t)(e - b));
		const char* le = nl ? nl : e;
		const char* f[10];
		int nf = 0;
		f[nf++] = b;
		for (const char* p = b; p < le && nf < 10; ++p)
			if (*p == '\t' || *p == ' ') f[nf++] = p + 1;
		const char* next = nl ? nl + 1 : e;
		if (le == b) { b = next; continue; }
		if (nf < 9) { out.error = "error: malformed SAM record: `" + std::string(b, le) + "'\n"; break; }
		auto end_of = [&](int i) { return i + 1 < nf ? f[i + 1] - 1 : le; };
		long long flag, pos, mapq, mpos, isize;
		if (!parse_int(f[1], end_of(1), flag) || !parse_int(f[3], end_of(3), pos) || !parse_int(f[4], end_of(4), mapq)
		    || !parse_int(f[7], end_of(7), mpos) || !parse_int(f[8], end_of(8), isize)) {
			out.error = "error: malformed SAM record: `" + std::string(b, le) + "'\n";
			break;
		}
		b = next;
		pos--;
		const char* q0 = f[0]; const char* q1 = end_of(0);
		if (q1 - q0 >= 2 && q1[-2] == '/' && (q1[-1] == '1' || q1[-1] == '2' || q1[-1] == '3')) flag |= 1; // paired
		const Cigar cg = parse_cigar(f[5], end_of(5));
		if (!cg.ok) { out.error = "error: invalid CIGAR: `" + std::string(f[5], end_of(5)) + "'\n"; break; }
		if (cg.qspan < opt.min_align || cg.tspan < opt.min_align) flag |= 4; // unmapped
		const char* r0 = f[2]; const char* r1 = end_of(2);
		const char* m0 = f[6]; const char* m1 = end_of(6);
		const bool same = (m1 - m0 == 1 && *m0 == '=') || ((m1 - m0) == (r1 - r0) && !memcmp(m0, r0, (size_t)(r1 - r0)));
		if ((flag & 4) || (flag & 8) || !(flag & 1) || same || (unsigned short)mapq < opt.min_mapq) continue;
		Rec x;
		if (!lookup(r0, r1, x.r)) { out.error = "error: unexpected ID: `" + std::string(r0, r1) + "'\n"; break; }
		name.assign(m0, m1);
		auto it = run.index.find(name);
		if (it == run.index.end()) { out.error = "error: unexpected ID: `" + name + "'\n"; break; }
		x.m = it->second;
		x.rev = (flag & 16) != 0;
		x.mrev = (flag & 32) != 0;
		x.a0 = x.rev ? (int)(pos + cg.tspan + (cg.qlen - cg.qspan - cg.qstart)) : (int)(pos - cg.qstart);
		x.a1 = x.a0 + (int)isize;
		out.recs.push_back(x);
	}
}

struct Input { // blocks of whole lines from a file or a pipe
	FILE* f;
	std::vector<char> buf;
	size_t have = 0;
	bool eof = false;
	explicit Input(FILE* f) : f(f) {}
	// fills buf with at least one whole line beyond what `keep` bytes hold (or everything left); returns the bytes of whole lines
	size_t fill(size_t block)
	{
		for (;;) {
			if (!eof) {
				if (buf.size() < have + block) buf.resize(have + block);
				const size_t got = fread(buf.data() + have, 1, block, f);
				have += got;
				if (got < block) eof = true;
			}
			if (eof) return have;
			for (size_t i = have; i > 0; --i)
				if (buf[i - 1] == '\n') return i;
		}
	}
	void consume(size_t n) { memmove(buf.data(), buf.data() + n, have - n); have -= n; }
};

inline int parse_options(int argc, char** argv, Options& opt, std::ostream& err, std::ostream& sout)
{
	static const char shortopts[] = "j:k:l:n:o:q:s:v";
	enum { O_HELP = 1, O_VERSION, O_MIND, O_MAXD, O_IGNORED };
	static int format, method, rf;
	format = FMT_DIST; method = M_MLE; rf = -1;
	static const struct option longopts[] = {
		{ "dist", no_argument, &format, FMT_DIST }, { "dot", no_argument, &format, FMT_DOT }, { "gv", no_argument, &format, FMT_DOT },
		{ "gfa", no_argument, &format, FMT_GFA2 }, { "gfa2", no_argument, &format, FMT_GFA2 }, { "fr", no_argument, &rf, 0 },
		{ "rf", no_argument, &rf, 1 }, { "min-align", required_argument, NULL, 'l' }, { "mind", required_argument, NULL, O_MIND },
		{ "maxd", required_argument, NULL, O_MAXD }, { "mle", no_argument, &method, M_MLE }, { "median", no_argument, &method, M_MEDIAN },
		{ "mean", no_argument, &method, M_MEAN }, { "kmer", required_argument, NULL, 'k' }, { "npairs", required_argument, NULL, 'n' },
		{ "out", required_argument, NULL, 'o' }, { "min-mapq", required_argument, NULL, 'q' }, { "seed-length", required_argument, NULL, 's' },
		{ "threads", required_argument, NULL, 'j' }, { "verbose", no_argument, NULL, 'v' }, { "help", no_argument, NULL, O_HELP },
		{ "version", no_argument, NULL, O_VERSION }, { "db", required_argument, NULL, O_IGNORED },
		{ "library", required_argument, NULL, O_IGNORED }, { "strain", required_argument, NULL, O_IGNORED },
		{ "species", required_argument, NULL, O_IGNORED }, { NULL, 0, NULL, 0 }
	};
	bool bad = false;
	optind = 1;
	for (int c; (c = getopt_long(argc, argv, shortopts, longopts, NULL)) != -1;) {
		std::istringstream arg(optarg != NULL ? optarg : "");
		std::string ignored;
		switch (c) {
		case '?': bad = true; break;
		case O_MIND: arg >> opt.min_dist; break;
		case O_MAXD: arg >> opt.max_dist; break;
		case 'l': arg >> opt.min_align; break;
		case 'j': arg >> opt.threads; break;
		case 'k': arg >> opt.k; break;
		case 'n': arg >> opt.npairs; break;
		case 'o': arg >> opt.out; break;
		case 'q': arg >> opt.min_mapq; break;
		case 's': arg >> opt.seed_len; break;
		case 'v': opt.verbose++; break;
		case O_HELP: sout << USAGE; return 0;
		case O_VERSION: sout << "DistanceEst (abyss_amd)\nA drop-in for ABySS's DistanceEst with the likelihood scan on the GPU.\n"; return 0;
		case O_IGNORED: arg >> ignored; break;
		}
		if (optarg != NULL && !arg.eof()) {
			err << "DistanceEst: invalid option: `-" << (char)c << optarg << "'\n";
			return 1;
		}
	}
	opt.format = format; opt.method = method; opt.rf = rf;
	if (opt.k <= 0) { err << "DistanceEst: missing -k,--kmer option\n"; bad = true; }
	if (opt.seed_len <= 0) { err << "DistanceEst: missing -s,--seed-length option\n"; bad = true; }
	if (opt.npairs <= 0) { err << "DistanceEst: missing -n,--npairs option\n"; bad = true; }
	if (argc - optind < 1) { err << "DistanceEst: missing arguments\n"; bad = true; }
	else if (argc - optind > 2) { err << "DistanceEst: too many arguments\n"; bad = true; }
	if (bad) { err << "Try `DistanceEst --help' for more information.\n"; return 1; }
	if (opt.seed_len < 2 * opt.k)
		err << "warning: the seed-length should be at least twice k: k=" << opt.k << ", s=" << opt.seed_len << '\n';
	if (opt.min_align == 0) { err << "DistanceEst: error: -l must be greater than zero\n"; return 1; }
	opt.hist = argv[optind++];
	if (argv[optind] != NULL) opt.sam = argv[optind++];
	opt.threads = std::max(1, std::min(16, opt.threads));
	return -1;
}

inline int run_main(int argc, char** argv, Backend& be, std::ostream& err = std::cerr, std::ostream& sout = std::cout)
{
	Run run(be, err);
	Options& opt = run.opt;
	const int st = parse_options(argc, argv, opt, err, sout);
	if (st >= 0) { sout.flush(); return st; }
	FILE* in = stdin;
	if (opt.sam != "-" && !(in = fopen(opt.sam.c_str(), "rb"))) { err << "error: `" << opt.sam << "': " << strerror(errno) << '\n'; return 1; }
	if (!opt.out.empty() && !(run.out = fopen(opt.out.c_str(), "wb"))) { err << "error: `" << opt.out << "': " << strerror(errno) << '\n'; return 1; }
	FILE* out = run.out;
	try {
		if (opt.format == FMT_DOT) fprintf(out, "digraph dist {\ngraph [k=%u s=%u n=%u]\n", opt.k, opt.seed_len, opt.npairs);
		else if (opt.format == FMT_GFA2) fputs("H\tVN:Z:2.0\n", out);

		// the histogram may not be there before the aligner has finished: wait for the first byte of the alignments
		Input input(in);
		size_t BLOCK = 32u << 20; // ABG_DE_BLOCK_BYTES: a test knob, so that small inputs reach the block seams; it changes no output
		if (const char* v = getenv("ABG_DE_BLOCK_BYTES")) BLOCK = std::max<size_t>(64, strtoull(v, nullptr, 10));
		const size_t PIECE = std::min<size_t>(1 << 16, std::max<size_t>(1, BLOCK / 4)); // the least a parser thread is started for
		size_t whole = input.fill(std::min<size_t>(1 << 16, BLOCK));

		Hist dh;
		{
			FILE* hf = fopen(opt.hist.c_str(), "rb");
			if (!hf) run.die("error: `" + opt.hist + "': " + strerror(errno) + "\n");
			long long v, c;
			while (fscanf(hf, "%lld %lld", &v, &c) == 2) dh.insert((int)v, (size_t)c);
			fclose(hf);
		}
		if (dh.empty()) run.die("error: the histogram `" + opt.hist + "' is empty\n");
		const unsigned num_rf = dh.count(INT_MIN, 0), num_fr = dh.count(1, INT_MAX), num_total = dh.size();
		const bool lib_rf = num_fr < num_rf;
		if (opt.verbose > 0)
			err << "Mate orientation FR: " << num_fr << std::setprecision(3) << " (" << (float)100 * num_fr / num_total << "%)"
			    << " RF: " << num_rf << std::setprecision(3) << " (" << (float)100 * num_rf / num_total << "%)\n"
			    << "The library " << opt.hist << " is oriented " << (lib_rf ? "reverse-forward (RF)" : "forward-reverse (FR)") << ".\n";
		if (opt.rf == -1) opt.rf = lib_rf;
		if (opt.rf) dh = dh.negate();
		if ((bool)opt.rf != lib_rf)
			err << "warning: The orientation is forced to " << (opt.rf ? "reverse-forward (RF)" : "forward-reverse (FR)")
			    << " which differs from the detected orientation.\n";
		dh.erase_negative();
		dh.remove_noise();
		dh.remove_outliers();
		const Hist h = dh.trim_fraction(0.0001);
		// Nothing left, as when the orientation is forced against the library: the reference goes on with a PMF of one entry whose
		// probabilities are 1 / 0, which no sample exceeds, so every estimate has no pair and none is written.
		run.no_pmf = h.empty();
		if (opt.verbose > 0)
			err << "Stats mean: " << std::setprecision(4) << h.mean() << " median: " << std::setprecision(4) << h.median()
			    << " sd: " << std::setprecision(4) << h.sd() << " n: " << h.size() << " min: " << h.minimum() << " max: " << h.maximum()
			    << '\n' << h.barplot() << std::endl;
		const Pmf pmf(h);
		run.pmf = &pmf;
		if (opt.min_dist == INT_MIN) opt.min_dist = -(int)opt.k + 1;
		if (opt.max_dist == INT_MAX) opt.max_dist = pmf.max_value();
		if (opt.verbose > 0) err << "Minimum and maximum distance are set to " << opt.min_dist << " and " << opt.max_dist << " bp.\n";
		if (!(opt.min_dist < opt.max_dist))
			run.die("DistanceEst: error: the minimum distance (" + std::to_string(opt.min_dist) + ") is not less than the maximum distance ("
			    + std::to_string(opt.max_dist) + ")\n");

		// the @SQ lines
		size_t at = 0;
		for (;;) {
			if (at == whole && !input.eof) { input.consume(at); at = 0; whole = input.fill(BLOCK); }
			if (at >= whole || input.buf[at] != '@') break;
			const char* b = input.buf.data() + at;
			const char* nl = (const char*)memchr(b, '\n', whole - at);
			const char* e = nl ? nl : input.buf.data() + whole;
			at = (size_t)(e - input.buf.data()) + (nl ? 1 : 0);
			std::istringstream ss(std::string(b, e));
			std::string type, sn, ln;
			ss >> type;
			if (type != "@SQ") continue;
			ss >> sn >> ln;
			char* end = nullptr;
			const unsigned long len = ln.compare(0, 3, "LN:") == 0 ? strtoul(ln.c_str() + 3, &end, 10) : 0;
			if (!ss || sn.compare(0, 3, "SN:") != 0 || sn.size() == 3 || !end || end == ln.c_str() + 3)
				run.die("DistanceEst: error: malformed @SQ line: `" + std::string(b, e) + "'\n");
			const std::string name = sn.substr(3);
			if (!run.index.insert({ name, (uint32_t)run.names.size() }).second) run.die("error: duplicate ID: `" + name + "'\n");
			run.names.push_back(name);
			run.lens.push_back((unsigned)len);
		}
		if (run.lens.empty()) run.die("error: no @SQ records in the SAM header\n");
		if (run.lens.size() == 1) { // one contig: no pair spans two
			fflush(out);
			return 0;
		}
		run.rec_ma = opt.min_align;
		std::vector<Rec> group;
		std::string stop; // why reading ended early
		while (stop.empty()) {
			if (at == whole) {
				if (input.eof) break;
				input.consume(at);
				at = 0;
				whole = input.fill(BLOCK);
				if (whole == 0) break;
			}
			// parse [at, whole) on the -j threads, pieces cut at line ends
			const char* base = input.buf.data();
			const unsigned nt = (unsigned)std::max<size_t>(1, std::min<size_t>((size_t)opt.threads, (whole - at) / PIECE));
			std::vector<size_t> cut(nt + 1, whole);
			cut[0] = at;
			for (unsigned t = 1; t < nt; ++t) {
				size_t p = at + (whole - at) * t / nt;
				const char* nl = (const char*)memchr(base + p, '\n', whole - p);
				cut[t] = std::max(cut[t - 1], nl ? (size_t)(nl - base) + 1 : whole);
			}
			std::vector<ParseOut> parsed(nt);
			std::vector<std::thread> pool;
			for (unsigned t = 1; t < nt; ++t) pool.emplace_back([&, t] { parse_lines(run, base + cut[t], base + cut[t + 1], parsed[t]); });
			parse_lines(run, base + cut[0], base + cut[1], parsed[0]);
			for (auto& t : pool) t.join();
			at = whole;
			for (unsigned t = 0; t < nt && stop.empty(); ++t) {
				for (const Rec& x : parsed[t].recs) {
					if (!group.empty() && group.front().r != x.r) {
						if (x.r < group.front().r) {
							stop = "error: input must be sorted: saw `" + run.names[group.front().r] + "' before `" + run.names[x.r] + "'\n";
							group.clear();
							break;
						}
						run.process_group(group);
						group.clear();
					}
					group.push_back(x);
				}
				if (stop.empty() && !parsed[t].error.empty()) { stop = parsed[t].error; group.clear(); }
			}
		}
		if (!group.empty()) run.process_group(group);
		run.flush();
		if (!stop.empty()) run.die(stop);

		if (opt.verbose > 0) {
			const float prop = (float)100 * (unsigned)run.dup_frags / (unsigned)run.total_frags;
			err << "Duplicate rate of spanning fragments: " << (unsigned)run.dup_frags << "/" << (unsigned)run.total_frags << " ("
			    << std::setprecision(3) << prop << "%)\n";
			if (prop > 50) err << "DistanceEst: warning: duplicate rate of fragments spanning more than one contig is high.\n";
		}
		if (opt.verbose > 0 && run.rec_ma != opt.min_align)
			err << "DistanceEst: warning: MLE will be more accurate if l is decreased to " << run.rec_ma << ".\n";
		if (opt.format == FMT_DOT) fputs("}\n", out);
		if (fflush(out) != 0 || (out != stdout && fclose(out) != 0)) { err << "DistanceEst: error: writing the output failed\n"; return 1; }
		return 0;
	} catch (const Die& d) {
		fflush(out);
		return d.status;
	}
}

// the backend over the serial bodies of abg_de.h: what the kernel must equal
struct SerialBackend : Backend {
	std::vector<double> pmf, logp;
	double minp = 0, mean = 0;
	bool open(std::string&) override { return true; }
	bool set_pmf(const std::vector<double>& p, double mp, double mn, std::string&) override
	{
		pmf = p;
		logp.resize(p.size());
		for (size_t i = 0; i < p.size(); ++i) logp[i] = log(p[i]);
		minp = mp;
		mean = mn;
		return true;
	}
	bool estimate(const std::vector<abg::DEPair>& pairs, const std::vector<int32_t>& samples, const std::vector<uint64_t>& off, int32_t* d,
	    uint32_t* n, std::string& err) override
	{
		const std::vector<double> hann = abg::de_hann(abg::de_filter_size(mean));
		std::vector<double> c, like, le;
		std::vector<uint32_t> cnt;
		for (size_t i = 0; i < pairs.size(); ++i) {
			abg::DEPrepared p;
			if (const char* why = abg::de_prepare(pairs[i], samples.data() + off[i], off[i + 1] - off[i], (int)pmf.size(), mean, p)) {
				err = "pair " + std::to_string(i) + ": " + why;
				return false;
			}
			const size_t t = p.job.last < p.job.first ? 0 : (size_t)((int64_t)p.job.last - p.job.first + 1);
			c.resize(t); like.resize(t); cnt.resize(t);
			abg::de_scan_job(p.job, p.values.data(), p.counts.data(), p.values.size(), pmf.data(), logp.data(), (int)pmf.size(), minp, log(minp),
			    c.data(), like.data(), cnt.data());
			int theta;
			abg::de_tail(p, hann, c.data(), like.data(), cnt.data(), le, theta, n[i]);
			d[i] = abg::de_finish(p, theta);
		}
		return true;
	}
};

} // namespace de
