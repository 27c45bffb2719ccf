// overlap_core.h -- host side of the drop-in `Overlap` (the rule abyss-pe runs after DistanceEst, bin/abyss-pe:658-659): options,
// the readers, the scaffold graph, the joins and the writers.  The one thing that touches the contigs' bytes in bulk -- which
// suffixes of t are prefixes of h, for every candidate pair -- is the caller's `Searcher` (abg_ov_* on the GPU in the product
// binary, include/abyss_amd.h; tests/hostcheck substitutes the same search body run serially).
//
// Reference behaviour restated here (ABySS 2.3.10):
//   Overlap/Overlap.cpp:38-126    messages and the option table; :365-425 the option loop and its errors
//   Overlap/Overlap.cpp:151-198   findOverlap: the -v line, none / too short / homopolymer / motif
//   Overlap/Overlap.cpp:212-261   the Overlap edge property, createGapContig
//   Overlap/Overlap.cpp:275-353   checkEdgeForOverlap (dot estimates), findOverlap (dist estimates)
//   Overlap/Overlap.cpp:427-598   main: readers, canonical edges, overlaps first, then scaffolds, the graph and the summary
//   Common/Estimate.h:71-104,154-198   DistanceEst's reader, allowedError, EstimateRecord
//   Graph/DotIO.h:16-113,159-309  the scaffold graph's dot reader and the -vv dot writer
//   Graph/ContigGraph.h:127-200, DirectedGraph.h:297-311,531-539   clear_out_edges, add_edge, remove_edge_if
//   Graph/ContigGraphAlgorithms.h:41-44   contiguous_out
//
// How it differs in structure: the reference searches a pair at the moment an estimate names it.  Whether an estimate can reach the
// search at all depends on things no search changes (the two ids, the distance and its error, the adjacency graph's degrees, the
// options), so a first pass over the estimates COLLECTS every distinct oriented pair that can; the matches of (t, h) and of
// (h^, t^) are the same set, so one of the two is kept.  The searcher answers them all at once.  A second pass REPLAYS the
// reference's loop in its order, looking answers up: the tests that do depend on earlier answers (an edge already in the scaffold
// graph, a masked pair under --no-merge-repeat leaving no edge so that its duplicate is searched and counted again) happen there
// exactly as in the reference, and the statistics are counted once per reference call.  Everything after the estimates is host
// graph work in the reference's order.
//
// Where the reference trips an assert, this prints an error naming the input and exits 1: an empty FASTA file, a distance of
// 100000 or more on a scaffolded edge, an estimate between a vertex and itself or its complement in a dot scaffold graph, a
// contig named by the graph that the FASTA file lacks, a contig shorter than k - 1 at a scaffolded end.  Colour-space contigs are
// refused.  The adjacency graph is read in the ADJ and GraphViz formats (contig_graph.h's readers).
#pragma once

#include "contig_graph.h"
#include "fasta_reader.h"
#include "host_cli.h"

#include <climits>
#include <cmath>
#include <getopt.h>

namespace ov {

#define ABG_OV_PROGRAM "Overlap"

using cg::V;
using abgio::ADJ; using abgio::ASQG; using abgio::DOT; using abgio::GFA1; using abgio::GFA2; using abgio::SAM;

static const char VERSION_MESSAGE[] =
    ABG_OV_PROGRAM " (ABySS) " ABG_IO_VERSION "\n"
    "Written by Shaun Jackman.\n"
    "\n"
    "Copyright 2014 Canada's Michael Smith Genome Sciences Centre\n";

static const char USAGE_MESSAGE[] =
    "Usage: " ABG_OV_PROGRAM " -k<kmer> -o<out.fa> [OPTION]... CONTIGS ADJ DIST\n"
    "Find overlaps between blunt contigs that have negative distance\n"
    "estimates. Add edges to the overlap graph.\n"
    "\n"
    " Options:\n"
    "\n"
    "  -k, --kmer=KMER_SIZE  k-mer size\n"
    "  -m, --min=OVERLAP     require a minimum of OVERLAP bases\n"
    "                        default is 5 bases\n"
    "      --scaffold        join contigs with Ns [default]\n"
    "      --no-scaffold     do not scaffold\n"
    "      --mask-repeat     join contigs at a simple repeat and mask\n"
    "                        the repeat sequence [default]\n"
    "      --no-merge-repeat don't join contigs at a repeat\n"
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
    "  -o, --out=FILE        write result to FILE\n"
    "  -v, --verbose         display verbose output\n"
    "      --help            display this help and exit\n"
    "      --version         output version information and exit\n"
    "\n"
    "Report bugs to <abyss-users@bcgsc.ca>.\n";

struct Options { // namespace opt, Overlap.cpp:77-97
	unsigned k = 0, minimum_overlap = 5;
	int mask = 1, scaffold = 1, ss = 0, format = ADJ, verbose = 0;
	std::string graphPath, out, commandLine, contigPath, adjPath, estPath;
};

// What the host asks of the search.  top[3 i ..] and ntop[i] as abg_ov_find gives them in top mode; in all mode every length.
struct Searcher {
	virtual ~Searcher() {}
	virtual bool open(std::string& err) = 0; // called once, and only when a pair has to be searched
	virtual bool set_contigs(const std::string& bytes, const std::vector<uint64_t>& offsets, std::string& err) = 0;
	virtual bool find(const std::vector<std::pair<V, V>>& pairs, bool all, std::vector<uint32_t>& top, std::vector<uint32_t>& ntop,
	    std::vector<uint64_t>& all_offsets, std::vector<uint32_t>& lengths, std::string& err) = 0;
};

// main's option loop, Overlap.cpp:376-425.  Returns false when the caller should exit with `*status`.
inline bool parse_options(int argc, char** argv, Options& o, int* status)
{
	o.commandLine = cli::command_line(argc, argv);
	enum { OPT_HELP = 1, OPT_VERSION };
	static int scaffold = 1, mask = 1, ss = 0, format = ADJ;
	static const struct option longopts[] = {
		{ "kmer", required_argument, NULL, 'k' }, { "min", required_argument, NULL, 'm' },
		{ "scaffold", no_argument, &scaffold, 1 }, { "no-scaffold", no_argument, &scaffold, 0 },
		{ "mask-repeat", no_argument, &mask, 1 }, { "no-merge-repeat", no_argument, &mask, 0 },
		{ "SS", no_argument, &ss, 1 }, { "no-SS", no_argument, &ss, 0 },
		{ "graph", required_argument, NULL, 'g' },
		{ "adj", no_argument, &format, ADJ }, { "asqg", no_argument, &format, ASQG }, { "dot", no_argument, &format, DOT },
		{ "gfa", no_argument, &format, GFA1 }, { "gfa1", no_argument, &format, GFA1 }, { "gfa2", no_argument, &format, GFA2 },
		{ "gv", no_argument, &format, DOT }, { "sam", no_argument, &format, SAM },
		{ "out", required_argument, NULL, 'o' }, { "verbose", no_argument, NULL, 'v' },
		{ "help", no_argument, NULL, OPT_HELP }, { "version", no_argument, NULL, OPT_VERSION },
		{ NULL, 0, NULL, 0 }
	};
	bool die = false;
	for (int c; (c = getopt_long(argc, argv, "g:k:m:o:v", longopts, NULL)) != -1;) {
		std::istringstream arg(optarg != NULL ? optarg : "");
		switch (c) {
		case '?': die = true; break;
		case 'g': arg >> o.graphPath; break;
		case 'k': arg >> o.k; break;
		case 'm': arg >> o.minimum_overlap; break;
		case 'o': arg >> o.out; break;
		case 'v': o.verbose++; break;
		case OPT_HELP: fputs(USAGE_MESSAGE, stdout); *status = EXIT_SUCCESS; return false;
		case OPT_VERSION: fputs(VERSION_MESSAGE, stdout); *status = EXIT_SUCCESS; return false;
		}
		if (optarg != NULL && !arg.eof()) {
			*status = cli::invalid_option(ABG_OV_PROGRAM, c, optarg);
			return false;
		}
	}
	o.scaffold = scaffold; o.mask = mask; o.ss = ss; o.format = format;
	if (o.k <= 0) { fprintf(stderr, ABG_OV_PROGRAM ": missing -k,--kmer option\n"); die = true; }
	if (o.out.empty()) { fprintf(stderr, ABG_OV_PROGRAM ": missing -o,--out option\n"); die = true; }
	if (argc - optind < 3) { fprintf(stderr, ABG_OV_PROGRAM ": missing arguments\n"); die = true; }
	if (argc - optind > 3) { fprintf(stderr, ABG_OV_PROGRAM ": too many arguments\n"); die = true; }
	if (die) {
		cli::try_help(ABG_OV_PROGRAM);
		*status = EXIT_FAILURE;
		return false;
	}
	o.contigPath = argv[optind++];
	o.adjPath = argv[optind++];
	o.estPath = argv[optind++];
	return true;
}

[[noreturn]] inline void fail(const std::string& msg) { cli::fail(ABG_OV_PROGRAM, msg); }

// DistanceEst (Estimate.h:26-38) with the two members Overlap adds (Overlap.cpp:212-237)
struct Est {
	int distance = 0;
	unsigned numPairs = 0;
	float stdDev = 0;
	unsigned overlap = UINT_MAX;
	bool mask = false;
};

// allowedError, Estimate.h:154-159 (opt::distanceError is 6)
inline unsigned allowed_error(float stddev) { return (unsigned)ceilf(3 * stddev + 6u); }

// ContigGraph<DirectedGraph<NoProperty, Overlap>>: out-edges in insertion order, vertex = 2 * contig + sense
struct SGraph {
	struct E { V v; Est ep; };
	std::vector<std::vector<E>> adj;
	explicit SGraph(size_t nv) : adj(nv) {}
	E* find(V u, V v) { for (E& e : adj[u]) if (e.v == v) return &e; return nullptr; }
	const E* find(V u, V v) const { for (const E& e : adj[u]) if (e.v == v) return &e; return nullptr; }
	bool has(V u, V v) const { return find(u, v) != nullptr; }
	void add1(V u, V v, const Est& ep) { adj[u].push_back(E{ v, ep }); }
	void add(V u, V v, const Est& ep) { add1(u, v, ep); if (u != (v ^ 1)) add1(v ^ 1, u ^ 1, ep); } // ContigGraph.h:190-200
	void remove1(V u, V v)
	{
		auto& e = adj[u];
		e.erase(std::remove_if(e.begin(), e.end(), [v](const E& x) { return x.v == v; }), e.end());
	}
	void clear_out_edges(V u) // ContigGraph.h:127-143
	{
		for (const E& e : adj[u]) if ((e.v ^ 1) != u) remove1(e.v ^ 1, u ^ 1);
		adj[u].clear();
	}
	void clear_in_edges(V v) { clear_out_edges(v ^ 1); }
	unsigned out_degree(V u) const { return (unsigned)adj[u].size(); }
	unsigned in_degree(V u) const { return (unsigned)adj[u ^ 1].size(); }
	bool contiguous_out(V u) const { return out_degree(u) == 1 && in_degree(adj[u][0].v) == 1; } // ContigGraphAlgorithms.h:41-44
	uint64_t num_edges() const { uint64_t n = 0; for (auto& a : adj) n += a.size(); return n; }
};

struct Stats { unsigned overlap = 0, scaffold = 0, none = 0, tooshort = 0, homopolymer = 0, motif = 0, ambiguous = 0; };

// one estimate as the reference meets it
struct DistCall { unsigned ref; bool rc; V pair; Est est; };

// operator>>(istream&, EstimateRecord&), Estimate.h:171-196, over a whole .dist file (SimpleGraph reads the same records):
// record(ref) for every record, then estimate(ref, rc, vertex, distance, numPairs, stdDev) for each of its estimates in file order.
// A name the graph lacks ends the run as Graph::find_contig does; `bad` is given the message for a malformed estimate.
template <class Record, class Estimate, class Bad>
inline void read_dist_records(const std::string& text, const cg::Graph& graph, const std::string& path, Record record, Estimate estimate, Bad bad)
{
	size_t p = 0;
	auto skip = [&]() { while (p < text.size() && isspace((unsigned char)text[p])) p++; };
	for (;;) {
		skip();
		if (p >= text.size()) break;
		size_t e = p;
		while (e < text.size() && !isspace((unsigned char)text[e])) e++;
		const unsigned ref = graph.find_contig(text.substr(p, e - p));
		record(ref);
		p = e;
		for (int rc = 0; rc <= 1; ++rc) {
			size_t end = text.find(rc ? '\n' : ';', p);
			if (end == std::string::npos) end = text.size();
			const std::string part = text.substr(p, end - p);
			p = std::min(text.size(), end + 1);
			size_t q = 0;
			for (;;) {
				while (q < part.size() && isspace((unsigned char)part[q])) q++;
				if (q >= part.size()) break;
				size_t comma = part.find(',', q);
				if (comma == std::string::npos) comma = part.size();
				const V v = graph.find_vertex(part.substr(q, comma - q));
				q = std::min(part.size(), comma + 1);
				// distance,numPairs,stdDev
				char* end1 = nullptr;
				const char* b = part.c_str() + q;
				const int distance = (int)strtol(b, &end1, 10);
				unsigned numPairs = 0;
				float stdDev = 0;
				bool ok = end1 != b && *end1 == ',';
				if (ok) { b = end1 + 1; numPairs = (unsigned)strtoul(b, &end1, 10); ok = end1 != b && *end1 == ','; }
				if (ok) { b = end1 + 1; stdDev = strtof(b, &end1); ok = end1 != b; }
				if (!ok) bad("`" + path + "': malformed estimate near `" + part.substr(q, 30) + "'");
				q = (size_t)(end1 - part.c_str());
				estimate(ref, rc != 0, v, distance, numPairs, stdDev);
			}
		}
	}
}

class Run {
  public:
	Run(Options& o, Searcher& s) : opt(o), searcher(s), scaffoldGraph(0) {}
	Options& opt;
	Searcher& searcher;
	cg::Graph graph;
	std::vector<std::string> contigs; // g_contigs
	SGraph scaffoldGraph;
	Stats stats;
	// the answers: per distinct pair its matching lengths, descending -- all of them under -v, else the first three
	std::map<std::pair<V, V>, size_t> index;
	std::vector<std::pair<V, V>> pairs;
	std::vector<std::vector<uint32_t>> answers;

	static std::pair<V, V> canonical(V t, V h)
	{
		const std::pair<V, V> a(t, h), b(h ^ 1, t ^ 1);
		return std::min(a, b);
	}
	void collect(V t, V h)
	{
		const auto key = canonical(t, h);
		if (index.emplace(key, pairs.size()).second) pairs.push_back(key);
	}
	std::string sequence(V u) const
	{
		const std::string& s = contigs[u >> 1];
		return (u & 1) ? cg::reverse_complement(s) : s;
	}

	void read_contigs()
	{
		abghost::ReaderOptions ro; // FastaReader::FOLD_CASE, Overlap.cpp:357
		abghost::FastaReader in(opt.contigPath, ro);
		std::string id, comment, s;
		while (in.read(id, comment, s)) contigs.push_back(s);
		if (contigs.empty()) fail("`" + opt.contigPath + "' holds no contigs");
		if (isdigit((unsigned char)contigs[0][0])) fail("`" + opt.contigPath + "' is in colour space, which this build does not read");
	}
	void read_graph()
	{
		cg::load_graph(opt.adjPath, opt.k, graph, fail);
		if (graph.nv() / 2 > contigs.size())
			fail("`" + opt.adjPath + "' names " + std::to_string(graph.nv() / 2) + " contigs and `" + opt.contigPath + "' holds " + std::to_string(contigs.size()));
	}

	// operator>>(istream&, DistanceEst&), Estimate.h:71-104, the GraphViz branch
	void read_dot_est(cg::Cursor& in, Est& o)
	{
		in.expect("d =");
		o.distance = in.integer("d");
		in.ws();
		if (in.peek() == ']') { o.stdDev = 0; o.numPairs = 0; return; }
		if (in.peek() == ',') { in.expect(", e ="); o.stdDev = real(in); in.expect(", n ="); o.numPairs = in.uns("n"); }
		else { in.expect(" e ="); o.stdDev = real(in); in.expect(" n ="); o.numPairs = in.uns("n"); }
	}
	static float real(cg::Cursor& in)
	{
		in.ws();
		char* end = nullptr;
		const float x = strtof(in.s.c_str() + in.p, &end);
		if (end == in.s.c_str() + in.p) cg::die("error: expected a number (e)");
		in.p = (size_t)(end - in.s.c_str());
		return x;
	}
	// read_dot (Graph/DotIO.h:159-309) on DirectedGraph<NoProperty, Overlap> with its vertices already there
	void read_dot_scaffold(const std::string& text)
	{
		cg::Cursor in(text);
		in.ws();
		in.expect("digraph");
		in.ignore('{');
		Est def;
		def.distance = -(int)opt.k + 1;
		for (bool done = false; !done;) {
			in.ws();
			if (in.eof()) break;
			switch (in.peek()) {
			case 'g':
				in.expect("graph [ ");
				if (in.peek() == 'k') {
					in.expect("k =");
					const unsigned k = in.uns("k");
					if (opt.k > 0 && k != opt.k) fail("`" + opt.estPath + "' was made with k=" + std::to_string(k) + ", not " + std::to_string(opt.k));
					opt.k = k;
				}
				in.ignore(']');
				break;
			case 'e':
				in.expect("edge [");
				in.ws();
				read_dot_est(in, def);
				in.ignore(']');
				break;
			default: done = true; break;
			}
			in.ws();
			if (in.peek() == ';') in.p++;
		}
		for (std::string uname; in.quoted(uname);) {
			in.ws();
			if (in.eof()) cg::die("error: unexpected end of the graph file");
			const char c = in.s[in.p++];
			if (c == ';') (void)graph.find_vertex(uname);
			else if (c == '[') { (void)graph.find_vertex(uname); in.ignore(']'); }
			else if (c == '-') {
				in.expect(">");
				const V u = graph.find_vertex(uname);
				in.ws();
				if (in.peek() == '{') {
					in.expect("{");
					for (std::string vn; in.quoted(vn);) scaffoldGraph.add1(u, graph.find_vertex(vn), def);
					in.expect(" }");
				} else {
					std::string vn;
					if (!in.quoted(vn)) { fprintf(stderr, "error: Expected `\"' and saw `%c'.\n", (char)in.peek()); exit(EXIT_FAILURE); }
					const V v = graph.find_vertex(vn);
					Est ep = def;
					in.ws();
					if (in.peek() == '[') { in.expect("["); in.ws(); read_dot_est(in, ep); in.ignore(']'); }
					if (const SGraph::E* e = scaffoldGraph.find(u, v)) { // DisallowParallelEdges, GraphIO.h:84-92
						fprintf(stderr, "error: parallel edges: [%s], [%s]\n", show(e->ep).c_str(), show(ep).c_str());
						exit(EXIT_FAILURE);
					}
					scaffoldGraph.add1(u, v, ep);
				}
			} else {
				fprintf(stderr, "error: Expected `[' or `->' and saw `%c'.\n", c);
				exit(EXIT_FAILURE);
			}
			in.ws();
			if (in.peek() == ';') in.p++;
		}
		in.expect("}");
		in.ws();
		if (!in.eof()) cg::die("error: Expected end-of-file after the graph");
	}
	// operator<<(ostream&, const Overlap&), Overlap.cpp:232-236
	static std::string show(const Est& o) { return "d=" + std::to_string(o.overlap > 0 ? -(int)o.overlap : o.distance); }

	// every estimate of the file in the order main meets them
	void read_dist(const std::string& text, std::vector<DistCall>& calls)
	{
		read_dist_records(text, graph, opt.estPath, [](unsigned) {},
		    [&](unsigned ref, bool rc, V v, int distance, unsigned numPairs, float stdDev) {
			    DistCall c;
			    c.ref = ref;
			    c.rc = rc;
			    c.pair = v;
			    c.est.distance = distance;
			    c.est.numPairs = numPairs;
			    c.est.stdDev = stdDev;
			    calls.push_back(c);
		    },
		    [](const std::string& msg) { fail(msg); });
	}

	// the answer for (t, h): overlaps, descending (the first three at least)
	const std::vector<uint32_t>& answer(V t, V h) const
	{
		auto it = index.find(canonical(t, h));
		if (it == index.end()) fail("internal: pair " + graph.vname(t) + " " + graph.vname(h) + " was not collected");
		return answers[it->second];
	}
	// findOverlap(g, t, h, mask), Overlap.cpp:151-198, after the loop
	unsigned judge(V t, V h, bool& mask)
	{
		mask = false;
		const std::vector<uint32_t>& overlaps = answer(t, h);
		if (opt.verbose > 0) {
			printf("%s\t%s", graph.vname(t).c_str(), graph.vname(h).c_str());
			for (uint32_t l : overlaps) printf("\t%u", l);
			putchar('\n');
		}
		if (overlaps.empty()) { stats.none++; return 0; }
		if (overlaps[0] < opt.minimum_overlap) { stats.tooshort++; return 0; }
		if (overlaps.size() >= 3 && overlaps[0] - overlaps[1] == overlaps[1] - overlaps[2]) {
			if (overlaps[0] - overlaps[1] == 1) stats.homopolymer++;
			else stats.motif++;
			mask = true;
		}
		return overlaps[0];
	}
	bool blunt(V t, V h) const { return !(graph.out_degree(t) > 0 || graph.in_degree(h) > 0); }
	static bool near(const Est& e) { return e.distance - (int)allowed_error(e.stdDev) <= 0; }

	// findOverlap(g, refID, rc, pair, est, out), Overlap.cpp:329-353; replay false: only collect the pair it could search
	void dist_call(const DistCall& c, bool replay)
	{
		if (c.ref == (c.pair >> 1) || (c.est.distance >= 0 && !opt.scaffold)) return;
		const V ref = 2 * c.ref;
		const V t = c.rc ? c.pair : ref, h = c.rc ? ref : c.pair;
		if (!blunt(t, h)) return;
		if (!replay) { if (near(c.est)) collect(t, h); return; }
		if (scaffoldGraph.has(t, h)) return;
		bool mask = false;
		const unsigned overlap = near(c.est) ? judge(t, h, mask) : 0;
		if (mask && !opt.mask) return;
		if (overlap > 0 || opt.scaffold) {
			Est ep = c.est;
			ep.overlap = overlap;
			ep.mask = mask;
			scaffoldGraph.add(t, h, ep);
		}
	}
	// checkEdgeForOverlap, Overlap.cpp:275-327, for the edge (u, v); ep is the edge's own property
	bool check_edge(V u, V v, bool replay)
	{
		if (u == v || u == (v ^ 1)) fail("`" + opt.estPath + "': an estimate joins " + graph.vname(u) + " and " + graph.vname(v));
		SGraph::E* e = scaffoldGraph.find(u, v);
		Est& ep = e->ep;
		if (replay && ep.overlap != UINT_MAX) return ep.overlap > 0 || opt.scaffold;
		if (ep.distance >= 0 && !opt.scaffold) return false;
		if (!blunt(u, v)) return false;
		if (!replay) { if (near(ep)) collect(u, v); return true; }
		bool mask = false;
		const unsigned overlap = near(ep) ? judge(u, v, mask) : 0;
		if (mask && !opt.mask) return false;
		if (overlap == 0 && !opt.scaffold) return false;
		ep.overlap = overlap;
		ep.mask = mask;
		const Est copy = ep;
		if (SGraph::E* c = scaffoldGraph.find(v ^ 1, u ^ 1)) c->ep = copy;
		else scaffoldGraph.add1(v ^ 1, u ^ 1, copy);
		return true;
	}
	// remove_edge_if(!checkEdgeForOverlap) on the plain directed graph, DirectedGraph.h:297-311,531-539
	void check_edges()
	{
		for (V u = 0; u < scaffoldGraph.adj.size(); ++u) {
			size_t out = 0;
			for (size_t it = 0; it < scaffoldGraph.adj[u].size(); ++it) {
				const V v = scaffoldGraph.adj[u][it].v;
				if (check_edge(u, v, true)) {
					auto& es = scaffoldGraph.adj[u];
					if (out != it) es[out] = es[it];
					++out;
				}
			}
			scaffoldGraph.adj[u].resize(out);
		}
	}

	void search()
	{
		if (pairs.empty()) return;
		std::string err;
		if (!searcher.open(err)) fail(err);
		std::string bytes;
		std::vector<uint64_t> off;
		cg::flatten(contigs, [](const std::string& s) -> const std::string& { return s; }, bytes, off);
		if (!searcher.set_contigs(bytes, off, err)) fail(err);
		const bool all = opt.verbose > 0;
		std::vector<uint32_t> top, ntop, lengths;
		std::vector<uint64_t> aoff;
		if (!searcher.find(pairs, all, top, ntop, aoff, lengths, err)) fail(err);
		answers.resize(pairs.size());
		for (size_t i = 0; i < pairs.size(); ++i) {
			if (all) answers[i].assign(lengths.begin() + aoff[i], lengths.begin() + aoff[i + 1]);
			else answers[i].assign(top.begin() + 3 * i, top.begin() + 3 * i + ntop[i]);
		}
	}

	// write_dot(out, scaffoldGraph), Graph/DotIO.h:16-113 for <NoProperty, Overlap>
	void dump_scaffold() const
	{
		printf("digraph adj {\n");
		if (opt.k > 0) printf("graph [k=%u]\nedge [d=%d]\n", opt.k, -(int)(opt.k - 1));
		for (V u = 0; u < scaffoldGraph.adj.size(); ++u) printf("\"%s\" []\n", graph.vname(u).c_str());
		for (V u = 0; u < scaffoldGraph.adj.size(); ++u)
			for (const SGraph::E& e : scaffoldGraph.adj[u]) {
				printf("\"%s\" -> \"%s\"", graph.vname(u).c_str(), graph.vname(e.v).c_str());
				if (e.ep.overlap != UINT_MAX) printf(" [%s]", show(e.ep).c_str()); // (ep == Overlap() compares the overlaps alone)
				putchar('\n');
			}
		printf("}\n");
	}

	int run()
	{
		read_contigs();
		read_graph();
		FILE* out = fopen(opt.out.c_str(), "wb");
		if (!out) { fprintf(stderr, "error: `%s': %s\n", opt.out.c_str(), strerror(errno)); return EXIT_FAILURE; }
		const std::string text = cg::slurp(opt.estPath);
		scaffoldGraph = SGraph(graph.nv());
		if (!text.empty() && text[0] == 'd') { // in.peek() == 'd', Overlap.cpp:451
			read_dot_scaffold(text);
			if (opt.verbose > 0) {
				std::map<int, uint64_t> h;
				for (auto& a : scaffoldGraph.adj) h[(int)a.size()]++;
				abgio::print_graph_stats(stdout, (unsigned)scaffoldGraph.adj.size(), (unsigned)scaffoldGraph.num_edges(), h);
			}
			for (V u = 0; u < scaffoldGraph.adj.size(); ++u)
				for (const SGraph::E& e : scaffoldGraph.adj[u]) check_edge(u, e.v, false);
			search();
			check_edges();
		} else {
			std::vector<DistCall> calls;
			read_dist(text, calls);
			for (const DistCall& c : calls) dist_call(c, false);
			search();
			for (const DistCall& c : calls) dist_call(c, true);
		}
		if (opt.verbose > 1) dump_scaffold();

		// Overlap.cpp:492-517: the canonical edges and the overlap subgraph
		SGraph overlapGraph(graph.nv());
		std::vector<std::pair<V, V>> edges;
		for (V u = 0; u < scaffoldGraph.adj.size(); ++u)
			for (const SGraph::E& e : scaffoldGraph.adj[u]) {
				if (e.v < u) continue;
				edges.push_back({ u, e.v });
				if (e.ep.overlap > 0) overlapGraph.add(u, e.v, e.ep);
			}
		// :520-541: overlapping edges first
		for (auto& tv : edges) {
			const V t = tv.first, h = tv.second;
			const SGraph::E* e = overlapGraph.find(t, h);
			if (!e) continue;
			if (overlapGraph.contiguous_out(t)) {
				stats.overlap++;
				graph.add_edge(t, h, -(int)e->ep.overlap);
				scaffoldGraph.clear_out_edges(t);
				scaffoldGraph.clear_in_edges(h);
			} else
				stats.ambiguous++;
		}
		// :544-579: then the scaffolded ones
		for (auto& tv : edges) {
			const V t = tv.first, h = tv.second;
			const SGraph::E* e = scaffoldGraph.find(t, h);
			if (!e) continue;
			if (e->ep.overlap > 0) continue;
			if (!scaffoldGraph.contiguous_out(t)) { stats.ambiguous++; continue; }
			V t1 = t, h1 = h;
			if (opt.ss && (t & 1) && (h & 1)) { t1 = h ^ 1; h1 = t ^ 1; }
			// createGapContig, Overlap.cpp:240-261
			stats.scaffold++;
			const int distance = e->ep.distance;
			if (opt.verbose > 0) printf("%s\t%s\t(%d)\n", graph.vname(t1).c_str(), graph.vname(h1).c_str(), distance);
			if (distance >= 100000) fail("`" + opt.estPath + "': the distance between " + graph.vname(t1) + " and " + graph.vname(h1) + " is 100000 or more");
			const std::string useq = sequence(t1), vseq = sequence(h1);
			const unsigned ends = opt.k - 1;
			if (useq.size() < ends) fail("contig " + graph.vname(t1) + " is shorter than k - 1");
			const std::string seq = useq.substr(useq.size() - ends) + (distance <= 0 ? std::string("n") : std::string((size_t)distance, 'N')) + vseq.substr(0, ends);
			const std::string name = graph.create_name();
			fprintf(out, ">%s %zu 0 %s %s %d\n%s\n", name.c_str(), seq.size(), graph.vname(t1).c_str(), graph.vname(h1).c_str(), distance, seq.c_str());
			const V v = graph.add_vertex((unsigned)seq.size(), 0);
			graph.put_name(v, name);
			const int def = -(int)opt.k + 1; // Distance(), ContigProperties.h
			graph.add_edge(t1, v, def);
			graph.add_edge(v, h1, def);
		}
		if (fclose(out) != 0) { fprintf(stderr, "error: `%s': %s\n", opt.out.c_str(), strerror(errno)); return EXIT_FAILURE; }

		if (!opt.graphPath.empty()) {
			FILE* g = fopen(opt.graphPath.c_str(), "wb");
			if (!g) { fflush(stdout); fprintf(stderr, "error: `%s': %s\n", opt.graphPath.c_str(), strerror(errno)); return EXIT_FAILURE; }
			{
				abgio::Out o(g);
				abgio::write_graph(o, graph, opt.format, ABG_OV_PROGRAM, opt.commandLine);
			}
			if (fclose(g) != 0) { fflush(stdout); fprintf(stderr, "error: `%s': %s\n", opt.graphPath.c_str(), strerror(errno)); return EXIT_FAILURE; }
		}
		printf("Overlap: %u\nScaffold: %u\nNo overlap: %u\nInsignificant (<%ubp): %u\nHomopolymer: %u\nMotif: %u\nAmbiguous: %u\n", stats.overlap,
		    stats.scaffold, stats.none, opt.minimum_overlap, stats.tooshort, stats.homopolymer, stats.motif, stats.ambiguous);
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

} // namespace ov
