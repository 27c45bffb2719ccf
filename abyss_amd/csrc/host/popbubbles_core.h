// popbubbles_core.h -- host side of the drop-in `PopBubbles` (the rule abyss-pe runs for %-2.path, bin/abyss-pe:604-605): options,
// the graph, the discovery of bubbles, their tests, the popped list, and with -g the assembled paths and the graph written back.
// The one thing with arithmetic in it -- the global alignment of a bubble's branches -- is the caller's `Aligner` (abg_pb_* on the
// GPU in the product binary, include/abyss_amd.h; tests/hostcheck substitutes the same header's serial text).
//
// Reference behaviour restated here (ABySS 2.3.10):
//   PopBubbles/PopBubbles.cpp:94-163      options;  :543-730 main
//   PopBubbles/PopBubbles.cpp:173-219     getDistance, CompareCoverage, popBubble
//   PopBubbles/PopBubbles.cpp:236-304     getSequence, getLength, getAlignmentIdentity
//   PopBubbles/PopBubbles.cpp:309-398     popSimpleBubble;  :401-421 addDistance;  :424-485 longestPath, scaffoldBubble, popOrScaffoldBubble
//   PopBubbles/PopBubbles.cpp:488-541     filterGraph, removeContig
//   Graph/PopBubbles.h:17-122             topologicalSort, isBubble, discoverBubbles
//   Graph/DepthFirstSearch.h:13-71        the three passes: in-degree 0, not contiguous-in, the rest
//   Graph/ContigGraphAlgorithms.h:40-253  contiguous_out / in, assemble_if, merge, assemble, assemble_stranded (the first, copy_out_edges
//                                         and the graph itself are contig_graph.h's)
//   Common/ContigProperties.h:212-233     EdgeWeightMap;  Graph/GraphUtil.h:43-64 printGraphStats, which leaves the stream at two
//                                         significant digits: every float written to stderr after it shows them
// How it differs in structure: the reference aligns a bubble's branches when its loop reaches the bubble.  Here every bubble that
// passes the cheap tests on the graph as read is found first and all their alignments go out in one batch; the loop is then replayed
// in the reference's order and takes its identities from the answers.  Under --scaffold the loop adds edges as it goes, which can
// change a later bubble's tests: an alignment the replay asks for that was not collected goes out in a call of its own.
// Where the reference fails an assertion the drop-in prints a message and exits 1 (INTEGRATION.md section 11 lists the cases).
#pragma once

#include "contig_graph.h"
#include "fasta_reader.h"
#include "host_cli.h"

#include <climits>
#include <getopt.h>
#include <iomanip>
#include <iostream>
#include <set>

namespace pb {

#define ABG_PB_PROGRAM "PopBubbles"

using cg::V; using cg::Graph; using cg::show_float;
using abgio::ADJ; using abgio::ASQG; using abgio::DOT; using abgio::GFA1; using abgio::GFA2; using abgio::SAM;

static const char VERSION_MESSAGE[] =
    ABG_PB_PROGRAM " (ABySS) " ABG_IO_VERSION "\n"
    "Written by Shaun Jackman.\n"
    "\n"
    "Copyright 2014 Canada's Michael Smith Genome Sciences Centre\n";

static const char USAGE_MESSAGE[] =
    "Usage: " ABG_PB_PROGRAM " -k<kmer> [OPTION]... FASTA ADJ\n"
    "Identify and pop simple bubbles.\n"
    "\n"
    " Arguments:\n"
    "\n"
    "  FASTA  contigs in FASTA format\n"
    "  ADJ    contig adjacency graph\n"
    "\n"
    " Options:\n"
    "\n"
    "  -k, --kmer=N          k-mer size\n"
    "  -a, --branches=N      maximum number of branches, default: 2\n"
    "  -b, --bubble-length=N pop bubbles shorter than N bp\n"
    "                        default is 10000\n"
    "  -p, --identity=REAL   minimum identity, default: 0.9\n"
    "  -c, --coverage=REAL   remove contigs with mean k-mer coverage\n"
    "                        less than this threshold [0]\n"
    "      --scaffold        scaffold over bubbles that have\n"
    "                        insufficient identity\n"
    "      --no-scaffold     disable scaffolding [default]\n"
    "      --SS              expect contigs to be oriented correctly\n"
    "      --no-SS           no assumption about contig orientation [default]\n"
    "  -g, --graph=FILE      write the contig adjacency graph to FILE\n"
    "      --adj             output the graph in ADJ format [default]\n"
    "      --asqg            output the graph in ASQG format\n"
    "      --dot             output the graph in GraphViz format\n"
    "      --gfa             output the graph in GFA1 format\n"
    "      --gfa1            output the graph in GFA1 format\n"
    "      --gfa2            output the graph in GFA2 format\n"
    "      --gv              output the graph in GraphViz format\n"
    "      --sam             output the graph in SAM format\n"
    "      --bubble-graph    output a graph of the bubbles\n"
    "  -j, --threads=N       use N parallel threads [1]\n"
    "  -v, --verbose         display verbose output\n"
    "      --help            display this help and exit\n"
    "      --version         output version information and exit\n"
    "\n"
    "Report bugs to <abyss-users@bcgsc.ca>.\n";

struct Options { // namespace opt, PopBubbles.cpp:94-125
	unsigned k = 0, maxBranches = 2, maxLength = 10000;
	float identity = 0.9f, minCoverage = 0;
	int scaffold = 0, bubbleGraph = 0, format = ADJ, ss = 0, threads = 1, verbose = 0;
	std::string graphPath, commandLine, contigsPath, adjPath;
};

// What the host asks of the alignment: align(seqs) of Align/alignGlobal.h:75-90 for every group of branches (two or more each):
// the matches and the size of the consensus.
struct Aligner {
	virtual ~Aligner() {}
	virtual bool open(std::string& err) = 0; // called once, and only when a bubble has passed the cheap tests
	virtual bool align(const std::vector<std::vector<std::string>>& groups, std::vector<uint32_t>& matches, std::vector<uint32_t>& size, std::string& err) = 0;
};

// main's option loop, PopBubbles.cpp:546-618.  Returns false when the caller should exit with `*status`.
inline bool parse_options(int argc, char** argv, Options& o, int* status)
{
	o.commandLine = cli::command_line(argc, argv);
	enum { OPT_HELP = 1, OPT_VERSION };
	static int format = ADJ, scaffold = 0, bubbleGraph = 0, ss = 0;
	static const struct option longopts[] = {
		{ "branches", required_argument, NULL, 'a' }, { "bubble-length", required_argument, NULL, 'b' }, { "coverage", required_argument, NULL, 'c' },
		{ "bubble-graph", no_argument, &bubbleGraph, 1 }, { "graph", required_argument, NULL, 'g' },
		{ "adj", no_argument, &format, ADJ }, { "asqg", no_argument, &format, ASQG }, { "dot", no_argument, &format, DOT },
		{ "gfa", no_argument, &format, GFA1 }, { "gfa1", no_argument, &format, GFA1 }, { "gfa2", no_argument, &format, GFA2 },
		{ "gv", no_argument, &format, DOT }, { "sam", no_argument, &format, SAM },
		{ "kmer", required_argument, NULL, 'k' }, { "identity", required_argument, NULL, 'p' },
		{ "scaffold", no_argument, &scaffold, 1 }, { "no-scaffold", no_argument, &scaffold, 0 }, { "SS", no_argument, &ss, 1 }, { "no-SS", no_argument, &ss, 0 },
		{ "threads", required_argument, NULL, 'j' }, { "verbose", no_argument, NULL, 'v' },
		{ "help", no_argument, NULL, OPT_HELP }, { "version", no_argument, NULL, OPT_VERSION },
		{ NULL, 0, NULL, 0 }
	};
	bool die = false;
	for (int c; (c = getopt_long(argc, argv, "a:b:c:g:j:k:p:v", longopts, NULL)) != -1;) {
		std::istringstream arg(optarg != NULL ? optarg : "");
		switch (c) {
		case '?': die = true; break;
		case 'a': arg >> o.maxBranches; break;
		case 'b': arg >> o.maxLength; break;
		case 'c': arg >> o.minCoverage; break;
		case 'g': arg >> o.graphPath; break;
		case 'j': arg >> o.threads; break; // (parsed and, as in the reference, used by nothing)
		case 'k': arg >> o.k; break;
		case 'p': arg >> o.identity; break;
		case 'v': o.verbose++; break;
		case OPT_HELP: fputs(USAGE_MESSAGE, stdout); *status = EXIT_SUCCESS; return false;
		case OPT_VERSION: fputs(VERSION_MESSAGE, stdout); *status = EXIT_SUCCESS; return false;
		}
		if (optarg != NULL && !arg.eof()) {
			*status = cli::invalid_option(ABG_PB_PROGRAM, c, optarg);
			return false;
		}
	}
	o.format = format; o.scaffold = scaffold; o.bubbleGraph = bubbleGraph; o.ss = ss;
	if (o.k <= 0) { fprintf(stderr, ABG_PB_PROGRAM ": missing -k,--kmer option\n"); die = true; }
	if (argc - optind < 2) { fprintf(stderr, ABG_PB_PROGRAM ": missing arguments\n"); die = true; }
	if (argc - optind > 2) { fprintf(stderr, ABG_PB_PROGRAM ": too many arguments\n"); die = true; }
	if (die) {
		cli::try_help(ABG_PB_PROGRAM);
		*status = EXIT_FAILURE;
		return false;
	}
	o.contigsPath = argv[optind++];
	o.adjPath = argv[optind++];
	return true;
}

[[noreturn]] inline void fail(const std::string& msg) { cli::fail(ABG_PB_PROGRAM, msg); }

typedef std::vector<V> Bubble;

class Run {
  public:
	Run(Options& o, Aligner& a) : opt(o), aligner(a) {}
	Options& opt;
	Aligner& aligner;
	Graph g;
	std::vector<std::string> contigs; // g_contigs
	std::vector<unsigned> popped;     // g_popped
	struct { unsigned bubbles = 0, popped = 0, scaffold = 0, notSimple = 0, tooLong = 0, tooMany = 0, dissimilar = 0; } count;
	int precision = 6; // of the floats written to stderr
	bool opened = false;
	// the answers so far: the bubble's first vertex and its branches in stored order -> (matches, consensus size)
	std::map<std::vector<V>, std::pair<uint32_t, uint32_t>> answers;

	void graph_stats()
	{
		cg::print_graph_stats(stderr, g);
		precision = 2;
		if (g.nv() == g.num_removed()) { // (-c removed every contig: the reference goes on to its histogram of nothing, 0 / 0 four times)
			volatile unsigned n = 0;
			const std::string nan = show_float((float)100 * n / n, 2);
			fprintf(stderr, "Degree: \n        01234\n0: %s%% 1: %s%% 2-4: %s%% 5+: %s%% max: 0\n", nan.c_str(), nan.c_str(), nan.c_str(), nan.c_str());
		}
	}

	void read_graph()
	{
		if (opt.verbose > 0) fprintf(stderr, "Reading `%s'...\n", opt.adjPath.c_str());
		cg::load_graph(opt.adjPath, opt.k, g, fail);
		if (opt.verbose > 0) graph_stats();
	}

	void read_contigs()
	{
		if (opt.verbose > 0) fprintf(stderr, "Reading `%s'...\n", opt.contigsPath.c_str());
		abghost::ReaderOptions ro; // FastaReader::NO_FOLD_CASE; opt::trimMasked keeps its default
		ro.foldCase = 0;
		abghost::FastaReader in(opt.contigsPath, ro);
		std::string id, comment, s;
		while (in.read(id, comment, s)) {
			auto it = g.index.find(id);
			if (it == g.index.end()) continue;
			if (it->second != contigs.size())
				fail("`" + opt.contigsPath + "': contig `" + id + "' is record " + std::to_string(contigs.size()) + " here and vertex " + std::to_string(it->second) +
				    " of the graph: the two must be in the same order");
			contigs.push_back(s);
		}
		if (contigs.empty()) fail("`" + opt.contigsPath + "' holds no contig of the graph");
		if (!contigs[0].empty() && isdigit((unsigned char)contigs[0][0])) fail("`" + opt.contigsPath + "' is in colour space, which this build does not read");
	}

	// filterGraph, PopBubbles.cpp:503-532
	void filter_graph()
	{
		unsigned removedContigs = 0, removedKmer = 0;
		for (uint64_t ui = 0; ui < g.nv(); ui++) {
			const V u = (V)ui;
			if (g.removed(u)) continue;
			if (g.length[u] < opt.k) fail("contig `" + g.cname(u) + "' is shorter than k");
			const unsigned kmers = g.length[u] - opt.k + 1;
			if ((float)g.coverage[u] / kmers < opt.minCoverage) {
				removedContigs++;
				removedKmer += kmers;
				g.clear_vertex(u);
				g.remove_vertex(u);
				popped.push_back(u >> 1);
			}
		}
		if (opt.verbose > 0) {
			fprintf(stderr, "Removed %u k-mer in %u contigs with mean k-mer coverage less than %s.\n", removedKmer, removedContigs, show_float(opt.minCoverage, precision).c_str());
			graph_stats();
		}
	}

	// depthFirstSearch (DepthFirstSearch.h:13-71) with TopoVisitor: the vertices in the order they finish
	std::vector<V> finish_order() const
	{
		const uint64_t n = g.nv();
		std::vector<uint8_t> colour(n, 0);
		std::vector<V> order;
		order.reserve(n);
		std::vector<std::pair<V, size_t>> stack;
		auto visit = [&](V root) {
			colour[root] = 1;
			stack.push_back({ root, 0 });
			while (!stack.empty()) {
				const V u = stack.back().first;
				size_t& at = stack.back().second;
				if (at < g.adj[u].size()) {
					const V v = g.adj[u][at++].v;
					if (colour[v] == 0) { colour[v] = 1; stack.push_back({ v, 0 }); }
				} else {
					colour[u] = 2;
					order.push_back(u);
					stack.pop_back();
				}
			}
		};
		for (uint64_t u = 0; u < n; u++) if (colour[u] == 0 && g.in_degree((V)u) == 0) visit((V)u);
		for (uint64_t u = 0; u < n; u++) if (colour[u] == 0 && !cg::contiguous_in(g, (V)u)) visit((V)u);
		for (uint64_t u = 0; u < n; u++) if (colour[u] == 0) visit((V)u);
		return order;
	}

	// isBubble, Graph/PopBubbles.h:45-70
	bool is_bubble(const V* first, const V* last) const
	{
		if (last - first == 2) return false;          // unambiguous edge
		if (*first == (last[-1] ^ 1)) return false;   // palindrome
		std::set<V> targets(first, first + 1), sources(last - 1, last), bubble(first, last);
		for (const V* it = first; it != last - 1; ++it) for (const cg::Edge& e : g.adj[*it]) targets.insert(e.v);
		for (const V* it = first + 1; it != last; ++it) for (const cg::Edge& e : g.adj[*it ^ 1]) sources.insert(e.v ^ 1);
		return sources == bubble && targets == bubble;
	}

	// discoverBubbles, Graph/PopBubbles.h:75-122
	std::vector<Bubble> discover_bubbles() const
	{
		std::vector<V> topo = finish_order();
		std::reverse(topo.begin(), topo.end());
		std::vector<Bubble> bubbles;
		for (size_t first = 0; first < topo.size(); ++first) {
			int sum = (int)g.out_degree(topo[first]);
			if (sum < 2) continue;
			if (opt.verbose > 3) fprintf(stderr, "* %s\n", g.vname(topo[first]).c_str());
			for (size_t it = first + 1; it < topo.size(); ++it) {
				const unsigned indeg = g.in_degree(topo[it]), outdeg = g.out_degree(topo[it]);
				sum -= (int)indeg;
				if (opt.verbose > 3) fprintf(stderr, "%s\t%u\t%u\t%d\t%d\n", g.vname(topo[it]).c_str(), indeg, outdeg, sum, sum + (int)outdeg);
				if (indeg == 0 || sum < 0) break;
				if (sum == 0) {
					if (is_bubble(topo.data() + first, topo.data() + it + 1)) {
						if (opt.verbose > 3) fprintf(stderr, "good\n");
						bubbles.push_back(Bubble(topo.begin() + first, topo.begin() + it + 1));
						first = it - 1;
					}
					break;
				}
				if (outdeg == 0) break;
				sum += (int)outdeg;
			}
		}
		return bubbles;
	}

	// popSimpleBubble's tests up to the alignment (PopBubbles.cpp:313-343, 354, 364-378): 0 simple, else which counter it ends at
	enum { SIMPLE = 0, NOT_SIMPLE, TOO_MANY, TOO_LONG };
	int simple_tests(V v, V& tail, unsigned& minLength, unsigned& maxLength, bool upto_simple = false) const
	{
		const unsigned nbranches = g.out_degree(v);
		const V v1 = g.adj[v][0].v;
		if (g.out_degree(v1) != 1) return NOT_SIMPLE;
		tail = g.adj[v1][0].v;
		if (v == (tail ^ 1) || g.in_degree(tail) != nbranches) return NOT_SIMPLE;
		for (const cg::Edge& e : g.adj[v]) {
			if (g.out_degree(e.v) != 1 || g.in_degree(e.v) != 1) return NOT_SIMPLE;
			if (g.adj[e.v][0].v != tail) return NOT_SIMPLE;
		}
		if (upto_simple) return SIMPLE;
		if (nbranches > opt.maxBranches) return TOO_MANY;
		minLength = UINT_MAX;
		maxLength = 0;
		for (const cg::Edge& e : g.adj[v]) { minLength = std::min(minLength, g.length[e.v]); maxLength = std::max(maxLength, g.length[e.v]); }
		return maxLength >= opt.maxLength ? TOO_LONG : SIMPLE;
	}

	std::vector<V> key_of(V v) const
	{
		std::vector<V> key(1, v);
		for (const cg::Edge& e : g.adj[v]) key.push_back(e.v);
		return key;
	}

	// getAlignmentIdentity up to align(seqs), PopBubbles.cpp:258-299.  true: the branches, trimmed of their overlaps, are to be
	// aligned; false: max_identity is the answer.
	struct Lengths { int max_in_overlap, max_out_overlap; float max_identity; };
	bool before_alignment(V t, V v, Lengths& L, std::vector<std::string>* seqs) const
	{
		const size_t n = g.adj[t].size();
		std::vector<int> inDists(n), outDists(n), insertLens(n);
		for (size_t i = 0; i < n; i++) {
			const V b = g.adj[t][i].v;
			inDists[i] = g.dist(t, b);
			outDists[i] = g.dist(b, v);
			insertLens[i] = (int)((unsigned)inDists[i] + g.length[b] + (unsigned)outDists[i]);
		}
		L.max_in_overlap = -*std::min_element(inDists.begin(), inDists.end());
		L.max_out_overlap = -*std::min_element(outDists.begin(), outDists.end());
		if (L.max_in_overlap < 0 || L.max_out_overlap < 0) fail("the branches of the bubble at " + g.vname(t) + " do not overlap their neighbours");
		const int min_insert_len = *std::min_element(insertLens.begin(), insertLens.end()), max_insert_len = *std::max_element(insertLens.begin(), insertLens.end());
		L.max_identity = (float)(min_insert_len + L.max_in_overlap + L.max_out_overlap) / (max_insert_len + L.max_in_overlap + L.max_out_overlap);
		if (min_insert_len <= 0 || L.max_identity < opt.identity) return false;
		if (!seqs) return true;
		seqs->resize(n);
		for (size_t i = 0; i < n; i++) {
			const V b = g.adj[t][i].v;
			if ((b >> 1) >= contigs.size()) fail("`" + opt.contigsPath + "' lacks contig `" + g.cname(b) + "'");
			const std::string s = (b & 1) ? cg::reverse_complement(contigs[b >> 1]) : contigs[b >> 1];
			const int len = (int)s.size(), l = -inDists[i], r = -outDists[i];
			if (l < 0 || r < 0 || len <= l + r)
				fail("contig `" + g.cname(b) + "' of " + std::to_string(len) + " bases is no longer than its overlaps of " + std::to_string(l) + " and " + std::to_string(r));
			(*seqs)[i] = s.substr(l, len - l - r);
		}
		return true;
	}

	void run_alignments(const std::vector<std::vector<V>>& keys, const std::vector<std::vector<std::string>>& groups)
	{
		if (keys.empty()) return;
		std::string err;
		if (!opened && !aligner.open(err)) fail(err);
		opened = true;
		std::vector<uint32_t> matches, size;
		if (!aligner.align(groups, matches, size, err)) fail(err);
		for (size_t i = 0; i < keys.size(); i++) answers[keys[i]] = { matches[i], size[i] };
	}

	// every bubble that reaches align(seqs) on the graph as it is now, in one batch
	void collect(const std::vector<Bubble>& bubbles)
	{
		if (opt.identity == 0) return;
		std::vector<std::vector<V>> keys;
		std::vector<std::vector<std::string>> groups;
		std::set<std::vector<V>> seen;
		for (const Bubble& b : bubbles) {
			const V v = b.front();
			V tail;
			unsigned mn, mx;
			Lengths L;
			std::vector<std::string> seqs;
			if (simple_tests(v, tail, mn, mx) != SIMPLE || !before_alignment(v, tail, L, nullptr)) continue;
			std::vector<V> key = key_of(v);
			if (!seen.insert(key).second) continue;
			before_alignment(v, tail, L, &seqs);
			keys.push_back(std::move(key));
			groups.push_back(std::move(seqs));
		}
		run_alignments(keys, groups);
	}

	float alignment_identity(V t, V v)
	{
		Lengths L;
		if (!before_alignment(t, v, L, nullptr)) return L.max_identity;
		const std::vector<V> key = key_of(t);
		auto it = answers.find(key);
		if (it == answers.end()) { // (the graph has changed since the batch was collected)
			std::vector<std::string> seqs;
			before_alignment(t, v, L, &seqs);
			run_alignments({ key }, { seqs });
			it = answers.find(key);
		}
		const unsigned matches = it->second.first, consensusSize = it->second.second;
		return (float)(matches + L.max_in_overlap + L.max_out_overlap) / (consensusSize + L.max_in_overlap + L.max_out_overlap);
	}

	// popBubble, PopBubbles.cpp:196-219
	void pop_bubble(V v, V tail)
	{
		std::vector<V> sorted;
		for (const cg::Edge& e : g.adj[v]) sorted.push_back(e.v);
		std::sort(sorted.begin(), sorted.end(), [this](V a, V b) { return g.coverage[a] > g.coverage[b]; });
		if (opt.bubbleGraph) {
			printf("\"%s\" -> {", g.vname(v).c_str());
			for (V u : sorted) printf(" \"%s\"", g.vname(u).c_str());
			printf(" } -> \"%s\"\n", g.vname(tail).c_str());
		}
		for (size_t i = 1; i < sorted.size(); i++) popped.push_back(sorted[i] >> 1);
	}

	// popSimpleBubble, PopBubbles.cpp:309-398
	bool pop_simple_bubble(V v)
	{
		V tail = 0;
		unsigned minLength = 0, maxLength = 0;
		if (simple_tests(v, tail, minLength, maxLength, true) != SIMPLE) { count.notSimple++; return false; }
		if (opt.verbose > 2) {
			fprintf(stderr, "\n* %s ->", g.vname(v).c_str());
			for (const cg::Edge& e : g.adj[v]) fprintf(stderr, " %s", g.vname(e.v).c_str());
			fprintf(stderr, " -> %s\n", g.vname(tail).c_str());
		}
		const int verdict = simple_tests(v, tail, minLength, maxLength);
		if (verdict == TOO_MANY) {
			count.tooMany++;
			if (opt.verbose > 1) fprintf(stderr, "%u paths (too many)\n", g.out_degree(v));
			return false;
		}
		if (verdict == TOO_LONG) {
			count.tooLong++;
			if (opt.verbose > 1) fprintf(stderr, "%u\t%u\t0\t(too long)\n", minLength, maxLength);
			return false;
		}
		const float identity = opt.identity == 0 ? 0 : alignment_identity(v, tail);
		const bool dissimilar = identity < opt.identity;
		if (opt.verbose > 1) fprintf(stderr, "%u\t%u\t%s%s\n", minLength, maxLength, show_float(identity, precision).c_str(), dissimilar ? "\t(dissimilar)" : "");
		if (dissimilar) { count.dissimilar++; return false; }
		count.popped++;
		pop_bubble(v, tail);
		return true;
	}

	// longestPath, PopBubbles.cpp:424-445 with EdgeWeightMap
	int longest_path(const Bubble& topo) const
	{
		std::map<V, int> distance;
		distance[topo.front()] = 0;
		for (V u : topo)
			for (const cg::Edge& e : g.adj[u]) {
				const int weight = e.d + (int)g.length[e.v];
				if (weight < 0) fail("invalid edge: " + g.vname(u) + " -> " + g.vname(e.v) + " [d=" + std::to_string(e.d) + "]");
				const int du = distance[u];
				int& dv = distance[e.v];
				dv = std::max(dv, du + weight);
			}
		return distance[topo.back()] - (int)g.length[topo.back()];
	}

	// scaffoldBubble, PopBubbles.cpp:451-472
	void scaffold_bubble(const Bubble& bubble)
	{
		const V u = bubble.front(), w = bubble.back();
		if (g.has_edge(u, w)) return; // already scaffolded
		if (!is_bubble(bubble.data(), bubble.data() + bubble.size())) fail("the bubble at " + g.vname(u) + " is no bubble any more");
		for (size_t i = 1; i + 1 < bubble.size(); i++) popped.push_back(bubble[i] >> 1);
		g.add_edge(u, w, std::max(longest_path(bubble), 1));
	}

	// assemble_if over the whole graph (ContigGraphAlgorithms.h:194-216) with pred0 = True (assemble) or IsPositive (assemble_stranded)
	std::vector<std::vector<V>> assemble()
	{
		std::vector<std::vector<V>> paths;
		auto pred = [this](V u, V v) { return u != (v ^ 1) && (!opt.ss || (!(u & 1) && !(v & 1))); };
		const uint64_t nv0 = g.nv();
		for (uint64_t ui = 0; ui < nv0; ui++) {
			V u = (V)ui;
			if (!cg::contiguous_out(g, u) || cg::contiguous_in(g, u) || !pred(u, g.adj[u][0].v)) continue;
			std::vector<V> path;
			while (cg::contiguous_out(g, u)) {
				const V v = g.adj[u][0].v;
				if (!pred(u, v)) break;
				path.push_back(u);
				u = v;
			}
			path.push_back(u);
			unsigned l = g.length[path[0]], c = g.coverage[path[0]]; // addProp
			for (size_t i = 1; i < path.size(); i++) {
				l += (unsigned)g.dist(path[i - 1], path[i]);
				l += g.length[path[i]];
				c += g.coverage[path[i]];
			}
			const V nu = g.add_vertex(l, c); // merge
			cg::copy_out_edges(g, path.front() ^ 1, nu ^ 1);
			cg::copy_out_edges(g, path.back(), nu);
			for (V x : path) g.clear_vertex(x);
			for (V x : path) g.remove_vertex(x);
			paths.push_back(path);
		}
		return paths;
	}

	int run()
	{
		read_graph();
		if (opt.identity > 0) read_contigs();
		if (opt.minCoverage > 0) filter_graph();
		if (opt.bubbleGraph) printf("digraph bubbles {\n");

		const std::vector<Bubble> bubbles = discover_bubbles();
		collect(bubbles);
		for (const Bubble& b : bubbles) { // popOrScaffoldBubble
			count.bubbles++;
			if (!pop_simple_bubble(b.front()) && opt.scaffold) {
				count.scaffold++;
				scaffold_bubble(b);
			}
		}

		// Each bubble should be identified twice. Remove the duplicate.
		std::sort(popped.begin(), popped.end());
		popped.erase(std::unique(popped.begin(), popped.end()), popped.end());
		if (opt.bubbleGraph) printf("}\n");
		else for (unsigned id : popped) printf("%s\n", g.names[id].c_str());

		if (opt.verbose > 0)
			fprintf(stderr, "Bubbles: %u Popped: %u Scaffolds: %u Complex: %u Too long: %u Too many: %u Dissimilar: %u\n", (count.bubbles + 1) / 2, (count.popped + 1) / 2,
			    (count.scaffold + 1) / 2, (count.notSimple + 1) / 2, (count.tooLong + 1) / 2, (count.tooMany + 1) / 2, (count.dissimilar + 1) / 2);

		if (!opt.graphPath.empty()) {
			for (unsigned id : popped) { g.clear_vertex(2 * id); g.remove_vertex(2 * id); } // removeContig
			const uint64_t numContigs = g.nv() / 2;
			Graph gorig;
			if (opt.scaffold) gorig = g;
			const std::vector<std::vector<V>> paths = assemble();
			for (size_t i = 0; i < paths.size(); i++) {
				const std::string name = g.create_name();
				g.put_name((V)(2 * (numContigs + i)), name);
				std::string line = name + '\t';
				const std::vector<V>& path = paths[i];
				line += g.vname(path[0]);
				for (size_t j = 1; j < path.size(); j++) {
					if (opt.scaffold) { // addDistance, PopBubbles.cpp:401-421
						const int distance = gorig.dist(path[j - 1], path[j]);
						if (distance >= 0) line += ' ' + std::to_string(std::max(distance + (int)opt.k - 1, 1)) + 'N';
					}
					line += ' ' + g.vname(path[j]);
				}
				printf("%s\n", line.c_str());
			}
			fflush(stdout);
			FILE* f = fopen(opt.graphPath.c_str(), "wb");
			if (!f) { fprintf(stderr, "error: `%s': %s\n", opt.graphPath.c_str(), strerror(errno)); exit(EXIT_FAILURE); }
			{
				abgio::Out o(f);
				abgio::write_graph(o, g, opt.format, ABG_PB_PROGRAM, opt.commandLine);
			}
			if (fclose(f) != 0) { fprintf(stderr, "error: `%s': %s\n", opt.graphPath.c_str(), strerror(errno)); exit(EXIT_FAILURE); }
			if (opt.verbose > 0) graph_stats();
		}
		fflush(stdout);
		return 0;
	}
};

inline int run_main(int argc, char** argv, Aligner& a)
{
	Options o;
	int status = 0;
	if (!parse_options(argc, argv, o, &status)) return status;
	Run r(o, a);
	return r.run();
}

} // namespace pb
