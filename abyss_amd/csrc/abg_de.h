// abg_de.h -- the maximum-likelihood distance estimate of DistanceEst (bin/abyss-pe:632-644): the scan over theta.
//
// Reference behaviour restated here (ABySS 2.3.10, paths relative to the repo):
//   DistanceEst/MLE.cpp:15-38    the window: (x <= 0 ? 1 : x < x1 ? x : x < x2 ? x1 : x < x3 ? x3 - x : 1) / (double)x1
//   DistanceEst/MLE.cpp:84-98    L(theta) = sum over the sample histogram, ascending, of n * log(pmf[x + theta]); n(theta) counts
//                                the samples with pmf[x + theta] > minProbability
//   DistanceEst/MLE.cpp:103-155  first/last are clamped and widened by half the filter; for every theta
//                                c(theta) = sum_{i=0..maxValue} pmf[i] * window(i - theta), likelihood = L - nsamples * log(c);
//                                a Hann filter over the likelihoods, then the arg max among thetas with n(theta) > 0
//   DistanceEst/MLE.cpp:164-211  len0, len1 lose l - 1 and are swapped into order; an FR sample loses 2(l - 1) and the estimate too
//   Common/PMF.h:29-32           an index outside [0, maxValue] reads minProbability: negative ones through the size_t conversion
//
// The split that makes the device's part bit-exact: the device computes c, L and n per theta with IEEE double adds, multiplies and
// divides in the reference's order and nothing else (this unit is compiled with -ffp-contract=off, so no product is fused into an
// add); every log is taken on the host: log(pmf[i]) once per PMF into a table, log(c) in the tail.  de_scan_job is that
// arithmetic run serially; the kernel of abg_de.hip uses the same de_window / de_c_term / de_like_step, tiled through LDS.
#pragma once
#include "abg_core.h"
#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

namespace abg {

constexpr int DE_BLOCK = 256; // thetas a workgroup at most
constexpr int DE_TILE = 2048; // PMF entries staged in LDS at a time
// thetas, sample values and the PMF's length stay within +-2^29 (the filter's margin included), so that i - theta and x + theta,
// which the reference computes in int, cannot overflow one
constexpr int DE_RANGE = 1 << 29;

struct DEJob { int32_t first, last; uint32_t len0, len1; };             // abg_de_job of include/abyss_amd.h
struct DEPair { int32_t first, last; uint32_t len0, len1, l, rf; };     // abg_de_pair of include/abyss_amd.h

ABG_HD double de_window(int x, int x1, int x2, int x3)
{
	return (x <= 0 ? 1 : x < x1 ? x : x < x2 ? x1 : x < x3 ? x3 - x : 1) / (double)x1;
}

ABG_HD double de_c_term(double c, double p, double w) { return c + p * w; }

// one sample (value x seen cnt times) of computeLikelihood
ABG_HD void de_like_step(double& like, unsigned& n, int x, unsigned cnt, int theta, const double* pmf, const double* logp, int npmf,
    double minp, double logminp)
{
	const int i = x + theta;
	const bool in = i >= 0 && i < npmf;
	const double p = in ? pmf[i] : minp;
	const double lp = in ? logp[i] : logminp;
	like += cnt * lp;
	if (p > minp) n += cnt;
}

// ---- host only from here: the serial scan, and the O(thetas) parts before and after it

// c, L and n of every theta of one job, serially: what the kernel must give bit for bit
inline void de_scan_job(const DEJob& j, const int32_t* sv, const uint32_t* sc, uint64_t ns, const double* pmf, const double* logp,
    int npmf, double minp, double logminp, double* c, double* like, uint32_t* n)
{
	const int x1 = (int)j.len0, x2 = (int)j.len1, x3 = (int)(j.len0 + j.len1);
	for (int64_t theta = j.first; theta <= j.last; ++theta) {
		double cs = 0;
		for (int i = 0; i < npmf; ++i) cs = de_c_term(cs, pmf[i], de_window(i - (int)theta, x1, x2, x3));
		double lk = 0;
		unsigned cnt = 0;
		for (uint64_t s = 0; s < ns; ++s) de_like_step(lk, cnt, sv[s], sc[s], (int)theta, pmf, logp, npmf, minp, logminp);
		c[theta - j.first] = cs;
		like[theta - j.first] = lk;
		n[theta - j.first] = cnt;
	}
}

// what one call of maximumLikelihoodEstimate turns into: the job, its sample histogram and what the tail needs
struct DEPrepared {
	DEJob job;
	std::vector<int32_t> values;
	std::vector<uint32_t> counts;
	uint32_t nsamples = 0;
	int filter = 3;
	int first = 0; // the caller's first: the floor of an FR estimate
	int shift = 0; // 2(l - 1) for FR
};

inline int de_filter_size(double mean) { return 2 * (int)(0.05 * mean) + 3; }

// MLE.cpp:164-211 up to the scan.  Returns NULL, or why the reference would have failed an assertion.
inline const char* de_prepare(const DEPair& p, const int32_t* samples, uint64_t ns, int npmf, double mean, DEPrepared& out)
{
	if (!(p.first < p.last)) return "the minimum distance is not less than the maximum distance";
	if (ns == 0) return "a contig pair has no samples";
	if (p.l == 0) return "the minimal alignment size is zero";
	if (p.len0 < p.l || p.len1 < p.l) return "a contig is shorter than the minimal alignment size (-l)";
	if (ns > 0xFFFFFFFFull) return "too many samples";
	if (p.first < -DE_RANGE || p.last > DE_RANGE) return "the distance bounds are out of range";
	uint32_t len0 = p.len0 - (p.l - 1), len1 = p.len1 - (p.l - 1);
	if (len0 > len1) std::swap(len0, len1);
	if ((uint64_t)len0 + len1 > 0x7FFFFFFFull) return "the contigs are too long";
	out.shift = p.rf ? 0 : 2 * (int)(p.l - 1);
	std::vector<int32_t> v(samples, samples + ns);
	if (!p.rf)
		for (auto& x : v) {
			if (!(x > out.shift)) return "an observed fragment is no longer than 2(l - 1), even after lowering l";
			x -= out.shift;
		}
	std::sort(v.begin(), v.end());
	out.values.clear();
	out.counts.clear();
	for (uint64_t i = 0; i < ns; ++i) {
		if (i && v[i] == v[i - 1]) out.counts.back()++;
		else { out.values.push_back(v[i]); out.counts.push_back(1); }
	}
	if (v.front() < -DE_RANGE || v.back() > DE_RANGE) return "a sample is out of range";
	out.nsamples = (uint32_t)ns;
	out.filter = de_filter_size(mean);
	out.first = p.first;
	const int smin = v.front(), smax = v.back();
	out.job.first = std::max(p.first, 0 - smax) - out.filter / 2;
	out.job.last = std::min(p.last, (npmf - 1) - smin) + out.filter / 2 + 1;
	out.job.len0 = len0;
	out.job.len1 = len1;
	if (out.job.first < -DE_RANGE || out.job.last > DE_RANGE) return "the distance bounds are out of range";
	return nullptr;
}

// MLE.cpp:40-75: the normalised zero-phase Hann window, weights[j + size / 2] for j in [-size / 2, size / 2]
inline std::vector<double> de_hann(int size)
{
	auto value = [size](int i) { return i < 0 || i >= size ? 0 : 0.5 * (1 - cos(2 * M_PI * i / (size - 1))); };
	double sum = 0;
	for (int i = 0; i < size; i++) sum += value(i);
	std::vector<double> w(2 * (size / 2) + 1);
	for (int j = -size / 2; j <= size / 2; j++) w[j + size / 2] = value(j + size / 2) / sum;
	return w;
}

// MLE.cpp:131-154 over the scan's arrays: (bestTheta, bestn) before the FR correction
inline void de_tail(const DEPrepared& p, const std::vector<double>& hann, const double* c, const double* like, const uint32_t* n,
    std::vector<double>& le, int& best_theta, uint32_t& best_n)
{
	const int64_t count = p.job.last < p.job.first ? 0 : (int64_t)p.job.last - p.job.first + 1;
	le.resize((size_t)count);
	for (int64_t i = 0; i < count; ++i) le[i] = like[i] - p.nsamples * log(c[i]);
	double best = -std::numeric_limits<double>::max();
	best_theta = p.job.first;
	best_n = 0;
	const int half = p.filter / 2;
	for (int i = half; i < (int)count - half; i++) {
		double likelihood = 0;
		for (int j = -half; j <= half; j++) likelihood += hann[j + half] * le[i + j];
		if (n[i] > 0 && likelihood > best) {
			best = likelihood;
			best_theta = p.job.first + i;
			best_n = n[i];
		}
	}
}

inline int de_finish(const DEPrepared& p, int best_theta) { return p.shift ? std::max(p.first, best_theta - p.shift) : best_theta; }

} // namespace abg
