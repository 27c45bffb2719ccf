// simplegraph_core.h -- host side of the drop-in `SimpleGraph` (the rule abyss-pe runs after Overlap, bin/abyss-pe:663-664): options,
// the readers, the pass over the estimates, the replay of handleEstimate and the summary.  The one thing that walks the graph in
// bulk -- the constrained depth-first search from every contig end that has estimates -- is the caller's `Searcher` (abg_sg_* on
// the GPU in the product binary, include/abyss_amd.h; tests/hostcheck substitutes the same search body run serially).
//
// Reference behaviour restated here (ABySS 2.3.10):
//   SimpleGraph/SimpleGraph.cpp:29-117    messages and the option table; :123-221 main
//   SimpleGraph/SimpleGraph.cpp:223-254   printConstraints, findRepeats
//   SimpleGraph/SimpleGraph.cpp:278-454   getDistance, calculatePathLength, constructAmbiguousPath, makeDistanceMap, printDistanceMap
//   SimpleGraph/SimpleGraph.cpp:461-650   handleEstimate
//   SimpleGraph/SimpleGraph.cpp:670-828   the worker loop (-s, -n, flipping the anterior estimates, the path line) and the summary
//   Common/Estimate.h:71-104,154-198      DistanceEst's reader and writer, allowedError, EstimateRecord
//   Common/ContigPath.h:19-45, ContigNode.h:41-48,215-232   reverseComplement, the path writer, the <n>N node
//   Graph/ContigGraphAlgorithms.h:100-111  extend
//
// How it differs in structure: the reference searches an end at the moment its record is read, on -j threads.  What a search is
// given (the origin, the constraint vertices and bounds, --max-cost) depends on nothing an earlier search found, so a first pass
// over the records filters them, flips the anterior estimates and COLLECTS every search, two a record at most; the searcher answers
// them all at once; a second pass REPLAYS the worker loop in input order, which is what -j1 writes.  -j is accepted and changes
// nothing.
//
// Where the reference aborts or trips an assert, this prints an error naming the input and exits 1: a name the graph lacks, a
// malformed estimate, an output file that cannot be opened.  The graph is read in the ADJ and GraphViz formats (contig_graph.h's
// readers); the others are refused.
#pragma once

#include "overlap_core.h"

#include <climits>
#include <cmath>
#include <cstdarg>
#include <map>
#include <set>

namespace sg {

#define ABG_SG_PROGRAM "SimpleGraph"

using cg::V; using cg::Node; using cg::Path;

static const char VERSION_MESSAGE[] =
    ABG_SG_PROGRAM " (ABySS) " ABG_IO_VERSION "\n"
    "Written by Jared Simpson and Shaun Jackman.\n"
    "\n"
    "Copyright 2018 Canada's Michael Smith Genome Sciences Centre\n";

static const char USAGE_MESSAGE[] =
    "Usage: " ABG_SG_PROGRAM " -k<kmer> -o<out.path> [OPTION]... ADJ DIST\n"
    "Find paths through contigs using distance estimates.\n"
    "\n"
    " Arguments:\n"
    "\n"
    "  ADJ   adjacency of the contigs\n"
    "  DIST  distance estimates between the contigs\n"
    "\n"
    " Options:\n"
    "\n"
    "  -k, --kmer=KMER_SIZE  k-mer size\n"
    "  -n, --npairs=N        minimum number of pairs [0]\n"
    "  -s, --seed-length=N   minimum seed contig length [0]\n"
    "  -d, --dist-error=N    acceptable error of a distance estimate\n"
    "                        default is 6 bp\n"
    "      --max-cost=COST   maximum computational cost\n"
    "  -o, --out=FILE        write result to FILE\n"
    "  -j, --threads=THREADS use THREADS parallel threads [1]\n"
    "      --extend          extend unambiguous paths\n"
    "      --no-extend       do not extend unambiguous paths [default]\n"
    "      --scaffold        join contigs with Ns [default]\n"
    "      --no-scaffold     do not scaffold\n"
    "  -v, --verbose         display verbose output\n"
    "      --help            display this help and exit\n"
    "      --version         output version information and exit\n"
    "      --db=FILE         specify path of database repository in FILE\n"
    "      --library=NAME    specify library NAME for sqlite\n"
    "      --strain=NAME     specify strain NAME for sqlite\n"
    "      --species=NAME    specify species NAME for sqlite\n"
    "\n"
    "Report bugs to <abyss-users@bcgsc.ca>.\n";

struct Options { // namespace opt, SimpleGraph.cpp:68-89 and ConstrainedSearch.h:16-21
	unsigned k = 0, threads = 1, minEdgeWeight = 0, minSeedLength = 0, distanceError = 6, maxCost = 100000;
	static constexpr unsigned maxPaths = 200;
	int extend = 0, scaffold = 1, verbose = 0;
	std::string out, adjPath, estPath;
};

// What the host asks of the search: for search i, from origins[i] under the constraints coff[i] .. coff[i + 1] (vertex, bound),
// the visit count and the paths index[i] .. index[i + 1], path p being nodes[poff[p] .. poff[p + 1]].
struct Searcher {
	virtual ~Searcher() {}
	virtual bool open(std::string& err) = 0; // called once, and only when there is a search to do
	virtual bool set_graph(const std::vector<uint64_t>& eoff, const std::vector<uint32_t>& lengths, const std::vector<uint32_t>& targets,
	    const std::vector<int32_t>& distances, std::string& err) = 0;
	virtual bool search(const std::vector<uint32_t>& origins, const std::vector<uint64_t>& coff, const std::vector<uint32_t>& cv,
	    const std::vector<int32_t>& cb, uint32_t max_cost, uint32_t max_paths, std::vector<uint32_t>& visited, std::vector<uint64_t>& index,
	    std::vector<uint64_t>& poff, std::vector<uint32_t>& nodes, std::string& err) = 0;
};

// main's option loop, SimpleGraph.cpp:128-189.  Returns false when the caller should exit with `*status`.
inline bool parse_options(int argc, char** argv, Options& o, int* status)
{
	enum { OPT_HELP = 1, OPT_VERSION, OPT_MAX_COST, OPT_DB, OPT_LIBRARY, OPT_STRAIN, OPT_SPECIES };
	static int extend = 0, scaffold = 1;
	static const struct option longopts[] = {
		{ "kmer", required_argument, NULL, 'k' }, { "npairs", required_argument, NULL, 'n' },
		{ "seed-length", required_argument, NULL, 's' }, { "dist-error", required_argument, NULL, 'd' },
		{ "max-cost", required_argument, NULL, OPT_MAX_COST }, { "out", required_argument, NULL, 'o' },
		{ "extend", no_argument, &extend, 1 }, { "no-extend", no_argument, &extend, 0 },
		{ "scaffold", no_argument, &scaffold, 1 }, { "no-scaffold", no_argument, &scaffold, 0 },
		{ "threads", required_argument, NULL, 'j' }, { "verbose", no_argument, NULL, 'v' },
		{ "help", no_argument, NULL, OPT_HELP }, { "version", no_argument, NULL, OPT_VERSION },
		{ "db", required_argument, NULL, OPT_DB }, { "library", required_argument, NULL, OPT_LIBRARY },
		{ "strain", required_argument, NULL, OPT_STRAIN }, { "species", required_argument, NULL, OPT_SPECIES },
		{ NULL, 0, NULL, 0 }
	};
	bool die = false;
	std::string ignored;
	for (int c; (c = getopt_long(argc, argv, "d:j:k:n:o:s:v", longopts, NULL)) != -1;) {
		std::istringstream arg(optarg != NULL ? optarg : "");
		switch (c) {
		case '?': die = true; break;
		case 'd': arg >> o.distanceError; break;
		case 'j': arg >> o.threads; break;
		case 'k': arg >> o.k; break;
		case OPT_MAX_COST: arg >> o.maxCost; break;
		case 'n': arg >> o.minEdgeWeight; break;
		case 'o': arg >> o.out; break;
		case 's': arg >> o.minSeedLength; break;
		case 'v': o.verbose++; break;
		case OPT_HELP: fputs(USAGE_MESSAGE, stdout); *status = EXIT_SUCCESS; return false;
		case OPT_VERSION: fputs(VERSION_MESSAGE, stdout); *status = EXIT_SUCCESS; return false;
		case OPT_DB: case OPT_LIBRARY: case OPT_STRAIN: case OPT_SPECIES: arg >> ignored; break; // (this build keeps no database)
		}
		if (optarg != NULL && !arg.eof()) {
			*status = cli::invalid_option(ABG_SG_PROGRAM, c, optarg);
			return false;
		}
	}
	o.extend = extend; o.scaffold = scaffold;
	if (o.k <= 0) { fprintf(stderr, ABG_SG_PROGRAM ": missing -k,--kmer option\n"); die = true; }
	if (o.out.empty()) { fprintf(stderr, ABG_SG_PROGRAM ": missing -o,--out option\n"); die = true; }
	if (argc - optind < 2) { fprintf(stderr, ABG_SG_PROGRAM ": missing arguments\n"); die = true; }
	else if (argc - optind > 2) { fprintf(stderr, ABG_SG_PROGRAM ": too many arguments\n"); die = true; }
	if (die) {
		cli::try_help(ABG_SG_PROGRAM);
		*status = EXIT_FAILURE;
		return false;
	}
	o.adjPath = argv[optind++];
	o.estPath = argv[optind++];
	return true;
}

[[noreturn]] inline void fail(const std::string& msg) { cli::fail(ABG_SG_PROGRAM, msg); }

struct Est { int distance = 0; unsigned numPairs = 0; float stdDev = 0; }; // DistanceEst, Estimate.h:26-38
typedef std::vector<std::pair<V, Est>> Estimates;
struct Record { unsigned ref = 0; Estimates est[2]; }; // EstimateRecord, Estimate.h:162-198

typedef std::vector<Path> Paths;

struct Stats { unsigned seedTooShort = 0, noEdges = 0, edgesRemoved = 0, totalAttempted = 0, uniqueEnd = 0, noPossiblePaths = 0, noValidPaths = 0,
	repeat = 0, multiEnd = 0, tooManySolutions = 0, tooComplex = 0; };

class Run {
  public:
	Run(Options& o, Searcher& s) : opt(o), searcher(s) {}
	Options& opt;
	Searcher& searcher;
	cg::Graph graph;
	Stats stats;
	unsigned minNumPairs = UINT_MAX, minNumPairsUsed = UINT_MAX; // g_minNumPairs, g_minNumPairsUsed
	FILE* out = nullptr;

	// the searches, in the order the replay meets them, and their answers
	std::vector<uint32_t> origins, cv, visited, nodes;
	std::vector<int32_t> cb;
	std::vector<uint64_t> coff{ 0 }, index, poff;
	size_t next = 0; // the replay's cursor into them

	// allowedError, Estimate.h:154-159
	unsigned allowed_error(float stddev) const { return (unsigned)ceilf(3 * stddev + opt.distanceError); }

	// the records of the .dist file, through the reader Overlap uses (overlap_core.h)
	void read_dist(const std::string& text, std::vector<Record>& records)
	{
		ov::read_dist_records(text, graph, opt.estPath, [&](unsigned ref) { records.emplace_back(); records.back().ref = ref; },
		    [&](unsigned, bool rc, V v, int distance, unsigned numPairs, float stdDev) {
			    Est est;
			    est.distance = distance;
			    est.numPairs = numPairs;
			    est.stdDev = stdDev;
			    records.back().est[rc].push_back({ v, est });
		    },
		    [](const std::string& msg) { fail(msg); });
	}

	std::string name(Node u) const { return cg::node_name(graph, u); }
	std::string show(const Path& p) const { return cg::show_path(graph, p); }
	static void appendf(std::string& s, const char* fmt, ...) __attribute__((format(printf, 2, 3)))
	{
		char buf[1024];
		va_list ap;
		va_start(ap, fmt);
		const int n = vsnprintf(buf, sizeof buf, fmt, ap);
		va_end(ap);
		s.append(buf, (size_t)std::min<int>(n, sizeof buf - 1));
	}

	int distance(Node u, Node v) const { return graph.dist((V)u, (V)v); } // getDistance, SimpleGraph.cpp:279-286
	// calculatePathLength, SimpleGraph.cpp:289-304
	unsigned path_length(Node origin, const Path& path, size_t prefix = 0, size_t suffix = 0) const
	{
		if (prefix + suffix == path.size()) return 0;
		int length = (int)graph.length[path[prefix]];
		for (size_t i = prefix + 1; i < path.size() - suffix; ++i) length += distance(path[i - 1], path[i]) + (int)graph.length[path[i]];
		const Node u = prefix == 0 ? origin : path[prefix - 1];
		length += distance(u, path[prefix]);
		return (unsigned)length;
	}
	// What all the paths agree on (constructAmbiguousPath, SimpleGraph.cpp:327-407): the vertices they share at the front, then, when
	// they also share some at the back, one ambiguous node as long as the middle of the longest path, then the shared back.  The
	// front is counted first and the back may not run into it, over the shortest path.
	Path ambiguous_path(Node origin, const Paths& paths) const
	{
		const Path& first = paths.front();
		size_t shortest = first.size();
		for (const Path& p : paths) shortest = std::min(shortest, p.size());
		auto all_have = [&](size_t from_front, bool back) {
			const Node want = back ? first[first.size() - 1 - from_front] : first[from_front];
			for (const Path& p : paths)
				if ((back ? p[p.size() - 1 - from_front] : p[from_front]) != want) return false;
			return true;
		};
		size_t front = 0;
		while (front < shortest && all_have(front, false)) ++front;
		size_t back = 0;
		while (back < shortest - front && all_have(back, true)) ++back;
		Path agreed(first.begin(), first.begin() + front);
		if (back == 0) return agreed;
		// the longest path, ties to the one of more vertices, the first of equals (max_element with ComparePathLength)
		const Path* longest = &paths.front();
		unsigned longest_length = path_length(origin, *longest);
		for (const Path& p : paths) {
			const unsigned l = path_length(origin, p);
			if (l > longest_length || (l == longest_length && p.size() > longest->size())) { longest = &p; longest_length = l; }
		}
		// its middle, from the end of the shared front to the start of the shared back, plus k - 1 by the convention of the path files
		const size_t first_of_back = longest->size() - back;
		const Node before_back = first_of_back == 0 ? origin : (*longest)[first_of_back - 1];
		const unsigned middle = path_length(origin, *longest, front, back) + (unsigned)distance(before_back, (*longest)[first_of_back]);
		const int gap = (int)(middle + opt.k - 1);
		if (gap <= 0) fail("the gap of an ambiguous path from " + name(origin) + " is not positive");
		agreed.push_back(-gap);
		agreed.insert(agreed.end(), first.end() - back, first.end());
		return agreed;
	}
	// Where each vertex of the path starts, measured from the end of the origin; a vertex the path holds twice has no one place and
	// is left out (makeDistanceMap, SimpleGraph.cpp:413-442)
	std::map<Node, int> distance_map(Node origin, const Path& path) const
	{
		std::map<Node, int> at;
		std::set<Node> twice;
		int d = 0;
		Node u = origin;
		for (const Node v : path) {
			d += distance(u, v);
			if (!at.insert({ v, d }).second) twice.insert(v);
			d += (int)graph.length[v];
			u = v;
		}
		for (const Node v : twice) at.erase(v);
		return at;
	}
	// extend, ContigGraphAlgorithms.h:100-111
	void extend(Path& path) const
	{
		V u = (V)path.back();
		std::set<V> seen;
		while (graph.out_degree(u) == 1 && seen.insert(u).second) {
			u = graph.adj[u][0].v;
			path.push_back((Node)u);
		}
	}

	// the first half of handleEstimate (SimpleGraph.cpp:475-485): the search of this end
	void collect(const Record& er, bool dir)
	{
		if (er.est[dir].empty()) return;
		origins.push_back(2 * er.ref + dir);
		for (const auto& e : er.est[dir]) {
			cv.push_back(e.first);
			cb.push_back((int32_t)((unsigned)e.second.distance + allowed_error(e.second.stdDev)));
		}
		coff.push_back(cv.size());
	}

	// handleEstimate, SimpleGraph.cpp:461-650, with the answer looked up
	void handle(const Record& er, bool dir, Path& outp)
	{
		const Estimates& ests = er.est[dir];
		if (ests.empty()) return;
		const size_t q = next++;
		const Node origin = (Node)(2 * er.ref + dir);
		const bool verbose = opt.verbose > 0;
		std::string vout;
		if (verbose) vout += "\n* " + name(origin) + "\n";
		unsigned minPairs = UINT_MAX;
		for (const auto& e : ests) minPairs = std::min(minPairs, e.second.numPairs);
		if (verbose) {
			vout += "Constraints:";
			for (uint64_t c = coff[q]; c < coff[q + 1]; ++c) appendf(vout, " %s,%d", name((Node)cv[c]).c_str(), cb[c]);
			vout += '\n';
		}
		Paths solutions;
		for (uint64_t p = index[q]; p < index[q + 1]; ++p) solutions.emplace_back(nodes.begin() + poff[p], nodes.begin() + poff[p + 1]);
		const bool tooComplex = visited[q] >= opt.maxCost;
		const bool tooManySolutions = solutions.size() > Options::maxPaths;

		// findRepeats, SimpleGraph.cpp:237-254
		std::set<unsigned> repeats;
		for (const Path& sol : solutions) {
			std::map<unsigned, unsigned> count;
			count[er.ref]++;
			for (Node u : sol) count[(unsigned)u >> 1]++;
			for (const auto& c : count) if (c.second > 1) repeats.insert(c.first);
		}
		if (verbose && !repeats.empty()) {
			vout += "Repeats:";
			for (unsigned id : repeats) vout += " " + graph.names[id];
			vout += '\n';
		}
		const unsigned numPossiblePaths = (unsigned)solutions.size();
		if (verbose && numPossiblePaths > 0) appendf(vout, "Paths: %u\n", numPossiblePaths);

		for (auto sol = solutions.begin(); sol != solutions.end();) {
			if (verbose) vout += show(*sol) + "\n";
			const std::map<Node, int> dm = distance_map(origin, *sol);
			unsigned validCount = 0, invalidCount = 0, ignoredCount = 0;
			for (const auto& e : ests) {
				const Node v = (Node)e.first;
				const Est& ep = e.second;
				if (verbose) { vout += name(v); appendf(vout, ",%d,%u,%.1f\t", ep.distance, ep.numPairs, (double)ep.stdDev); }
				const auto it = dm.find(v);
				if (it == dm.end()) { // this contig is a repeat
					ignoredCount++;
					if (verbose) vout += "ignored\n";
					continue;
				}
				const int actual = it->second;
				const int diff = actual - ep.distance;
				const unsigned buffer = allowed_error(ep.stdDev);
				const bool invalid = (unsigned)abs(diff) > buffer;
				const bool repeat = repeats.count((unsigned)v >> 1) > 0;
				const bool ignored = invalid && repeat;
				if (ignored) ignoredCount++;
				else if (invalid) invalidCount++;
				else validCount++;
				if (verbose) appendf(vout, "dist: %d diff: %d buffer: %u n: %u%s\n", actual, diff, buffer, ep.numPairs, ignored ? " ignored" : invalid ? " invalid" : "");
			}
			if (invalidCount == 0 && validCount > 0) ++sol;
			else sol = solutions.erase(sol);
		}

		if (verbose) {
			appendf(vout, "Solutions: %zu", solutions.size());
			if (tooComplex) vout += " (too complex)";
			if (tooManySolutions) vout += " (too many solutions)";
			vout += '\n';
		}
		size_t bestSol = solutions.size();
		int minDiff = 999999;
		for (size_t si = 0; si < solutions.size(); ++si) {
			const std::map<Node, int> dm = distance_map(origin, solutions[si]);
			int sumDiff = 0;
			for (const auto& e : ests) {
				if (repeats.count(e.first >> 1) > 0) continue;
				const auto it = dm.find((Node)e.first);
				if (it == dm.end()) fail("internal: " + name((Node)e.first) + " is on no path from " + name(origin));
				sumDiff += abs(it->second - e.second.distance);
			}
			if (sumDiff < minDiff) { minDiff = sumDiff; bestSol = si; }
			if (verbose) { vout += show(solutions[si]); appendf(vout, " length: %u sumdiff: %d\n", path_length(origin, solutions[si]), sumDiff); }
		}

		stats.totalAttempted++;
		minNumPairs = std::min(minNumPairs, minPairs);
		if (tooComplex) stats.tooComplex++;
		else if (tooManySolutions) stats.tooManySolutions++;
		else if (numPossiblePaths == 0) stats.noPossiblePaths++;
		else if (solutions.empty()) stats.noValidPaths++;
		else if (repeats.count(er.ref) > 0) {
			if (verbose) vout += "Repeat: " + name(origin) + "\n";
			stats.repeat++;
		} else if (solutions.size() > 1) {
			Path path = ambiguous_path(origin, solutions);
			if (!path.empty()) {
				if (opt.extend) extend(path);
				if (verbose) vout += show(path) + "\n";
				if (opt.scaffold) {
					outp.insert(outp.end(), path.begin(), path.end());
					minNumPairsUsed = std::min(minNumPairsUsed, minPairs);
				}
			}
			stats.multiEnd++;
		} else {
			if (bestSol >= solutions.size()) fail("internal: the one solution from " + name(origin) + " has a distance sum of 999999 or more");
			Path& path = solutions[bestSol];
			if (opt.verbose > 1) // printDistanceMap, SimpleGraph.cpp:445-454
				for (const auto& d : distance_map(origin, path)) appendf(vout, "\"%s\" -> \"%s\" [d=%d]\n", name(origin).c_str(), name(d.first).c_str(), d.second);
			if (opt.extend) extend(path);
			outp.insert(outp.end(), path.begin(), path.end());
			stats.uniqueEnd++;
			minNumPairsUsed = std::min(minNumPairsUsed, minPairs);
		}
		fputs(vout.c_str(), stdout);
	}

	void search()
	{
		if (origins.empty()) return;
		std::string err;
		if (!searcher.open(err)) fail(err);
		std::vector<uint64_t> eoff{ 0 };
		std::vector<uint32_t> targets;
		std::vector<int32_t> distances;
		for (uint64_t u = 0; u < graph.nv(); ++u) {
			for (const cg::Edge& e : graph.adj[u]) { targets.push_back(e.v); distances.push_back(e.d); }
			eoff.push_back(targets.size());
		}
		if (!searcher.set_graph(eoff, graph.length, targets, distances, err)) fail(err);
		if (!searcher.search(origins, coff, cv, cb, opt.maxCost, Options::maxPaths, visited, index, poff, nodes, err)) fail(err);
	}

	int run()
	{
		if (opt.verbose > 0) fprintf(stderr, "Reading `%s'...\n", opt.adjPath.c_str());
		cg::load_graph(opt.adjPath, opt.k, graph, fail);
		if (opt.verbose > 0) cg::print_graph_stats(stdout, graph);
		if (opt.verbose > 0) fprintf(stderr, "Reading `%s'...\n", opt.estPath.c_str());
		const std::string text = cg::slurp(opt.estPath);
		out = fopen(opt.out.c_str(), "wb");
		if (!out) { fflush(stdout); fprintf(stderr, "error: `%s': %s\n", opt.out.c_str(), strerror(errno)); return EXIT_FAILURE; }
		std::vector<Record> records;
		read_dist(text, records);

		// the worker loop's filters (SimpleGraph.cpp:685-709), once
		std::vector<char> skip(records.size(), 0);
		for (size_t i = 0; i < records.size(); ++i) {
			Record& er = records[i];
			if (graph.length[2 * er.ref] < opt.minSeedLength) { stats.seedTooShort++; skip[i] = 1; continue; }
			for (unsigned d = 0; d < 2; ++d) {
				Estimates& es = er.est[d];
				if (es.empty()) continue;
				const size_t before = es.size();
				es.erase(std::remove_if(es.begin(), es.end(), [&](const Estimates::value_type& e) { return e.second.numPairs < opt.minEdgeWeight; }), es.end());
				stats.edgesRemoved += (unsigned)(before - es.size());
				if (es.empty()) stats.noEdges++;
			}
			for (auto& e : er.est[1]) e.first ^= 1; // flip the anterior distance estimates
			collect(er, true);
			collect(er, false);
		}
		search();
		for (size_t i = 0; i < records.size(); ++i) {
			if (skip[i]) continue;
			const Record& er = records[i];
			Path path;
			handle(er, true, path);
			std::reverse(path.begin(), path.end()); // reverseComplement, ContigPath.h:19-25
			for (Node& u : path) if (u >= 0) u ^= 1;
			path.push_back((Node)(2 * er.ref));
			handle(er, false, path);
			if (path.size() > 1) fprintf(out, "%s\t%s\n", graph.names[er.ref].c_str(), show(path).c_str());
		}
		if (opt.verbose > 0) putchar('\n');
		printf("Seed too short: %u\nSeeds with no edges: %u\nEdges removed: %u\nTotal paths attempted: %u\nUnique path: %u\nNo possible paths: %u\n"
		       "No valid paths: %u\nRepetitive: %u\nMultiple valid paths: %u\nToo many solutions: %u\nToo complex: %u\n",
		    stats.seedTooShort, stats.noEdges, stats.edgesRemoved, stats.totalAttempted, stats.uniqueEnd, stats.noPossiblePaths, stats.noValidPaths,
		    stats.repeat, stats.multiEnd, stats.tooManySolutions, stats.tooComplex);
		if (fclose(out) != 0) { fflush(stdout); fprintf(stderr, "error: `%s': %s\n", opt.out.c_str(), strerror(errno)); return EXIT_FAILURE; }
		printf("\nThe minimum number of pairs in a distance estimate is %u.\n", minNumPairs);
		if (minNumPairsUsed != UINT_MAX) {
			printf("The minimum number of pairs used in a path is %u.\n", minNumPairsUsed);
			if (minNumPairs < minNumPairsUsed) printf("Consider increasing the number of pairs threshold parameter, n, to %u.\n", minNumPairsUsed);
		}
		return 0;
	}
};

inline int run_main(int argc, char** argv, Searcher& s)
{
	Options o;
	int status = 0;
	if (!parse_options(argc, argv, o, &status)) return status;
	Run r(o, s);
	return r.run();
}

} // namespace sg
