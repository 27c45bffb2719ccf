// mergecontigs_core.h -- host side of the drop-in `MergeContigs` (bin/abyss-pe:600, 608, 680, 689, 746, 839, 892): options, the
// readers, the FASTA and graph writers and the summary.  The one thing that touches the contigs' bytes in bulk -- splicing every
// path of two or more nodes into a sequence -- is the caller's `Merger` (abg_mc_* on the GPU in the product binary,
// include/abyss_amd.h; tests/hostcheck substitutes the serial text of the same abg_mc.h).
//
// Reference behaviour restated here (ABySS 2.3.10):
//   MergePaths/MergeContigs.cpp:38-136    messages and the option table; :434-661 main
//   MergePaths/MergeContigs.cpp:206-313   the vertex bundle of a gap, the junction's distance, pathToComment, mergePath's coverage
//   MergePaths/MergeContigs.cpp:321-432   readPaths, seenContigs, markRemovedContigs, outputGraph
//   Common/ContigNode.h:286-304, ContigPath.h:37-60   find_vertex and the path reader and writer
//   Common/ContigProperties.h:86-106,187-208   the vertex property as --dot-meancov prints it; the edge of a junction
//   Graph/ContigGraphAlgorithms.h:54-190  copy_out_edges, copy_in_edges, remove_vertex_if, addProp, merge
//   Common/Histogram.h:320-374, StringUtil.h:122-136   printContiguityStats, toEng
//
// How it differs in structure: the reference merges a path at the moment it writes it.  A junction's overlap depends on the graph
// alone, so a first pass looks every junction up; the merger splices all paths in one call; the writer then goes through the paths
// in input order.  Where a junction fails the reference's assert, the paths before it are still merged and their warnings printed
// before the error, as the reference's stderr has them.
//
// Where the reference aborts or trips an assert, this prints an error naming the input and exits 1: a path edge the graph lacks
// (after the reference's own `error: no edge` line), an edge of distance >= 0 on a path, a FASTA file whose order differs from the
// graph's, an empty FASTA file, colour-space contigs, a malformed node name.  The graph is read in the ADJ and GraphViz formats
// (contig_graph.h's readers); the others are refused.  --db, --library, --strain and --species are accepted and ignored.
#pragma once

#include "contig_graph.h"
#include "fasta_reader.h"
#include "host_cli.h"

#include <cmath>
#include <getopt.h>
#include <iomanip>
#include <iostream>
#include <limits>

namespace mc {

#define ABG_MC_PROGRAM "MergeContigs"

using cg::V; using cg::Node; using cg::Path; using cg::show_float;
using abgio::ADJ; using abgio::DOT; using abgio::GFA1; using abgio::GFA2; using abgio::SAM;
enum { DOT_MEANCOV = 100 };

static const char VERSION_MESSAGE[] =
    ABG_MC_PROGRAM " (ABySS) " ABG_IO_VERSION "\n"
    "Written by Shaun Jackman.\n"
    "\n"
    "Copyright 2014 Canada's Michael Smith Genome Sciences Centre\n";

static const char USAGE_MESSAGE[] =
    "Usage: " ABG_MC_PROGRAM " -k<kmer> -o<out.fa> [OPTION]... FASTA [OVERLAP] PATH\n"
    "Merge paths of contigs to create larger contigs.\n"
    "\n"
    " Arguments:\n"
    "\n"
    "  FASTA    contigs in FASTA format\n"
    "  OVERLAP  contig overlap graph\n"
    "  PATH     sequences of contig IDs\n"
    "\n"
    " Options:\n"
    "\n"
    "  -k, --kmer=KMER_SIZE  k-mer size\n"
    "  -o, --out=FILE        output the merged contigs to FILE [stdout]\n"
    "  -g, --graph=FILE      write the contig overlap graph to FILE\n"
    "      --merged          output only merged contigs\n"
    "      --adj             output the graph in adj format\n"
    "      --dot             output the graph in dot format [default]\n"
    "      --dot-meancov     same as above but give the mean coverage\n"
    "      --gfa             output the graph in GFA1 format\n"
    "      --gfa1            output the graph in GFA1 format\n"
    "      --gfa2            output the graph in GFA2 format\n"
    "      --gv              output the graph in GraphViz format\n"
    "      --sam             output the graph in SAM format\n"
    "  -v, --verbose         display verbose output\n"
    "      --help            display this help and exit\n"
    "      --version         output version information and exit\n"
    "      --db=FILE         specify path of database repository in FILE\n"
    "      --library=NAME    specify library NAME for database\n"
    "      --strain=NAME     specify strain NAME for database\n"
    "      --species=NAME    specify species NAME for database\n"
    "\n"
    "Report bugs to <abyss-users@bcgsc.ca>.\n";

struct Options { // namespace opt, MergeContigs.cpp:78-101
	unsigned k = 0;
	int format = DOT, onlyMerged = 0, verbose = 0;
	std::string out = "-", graphPath, commandLine, contigPath, adjPath, pathPath;
};

// What the host asks of the merge: path i is nodes[noff[i] .. noff[i + 1]], ov[j] the overlap of nodes[j] with what precedes it.
// Back come the sequences, seqs[soff[i] .. soff[i + 1]], their ACGT counts, and the stderr text of the paths merged the slow way,
// logs[loff[i] .. loff[i + 1]], with the placeholders of abg_mc.h for names.
struct Merger {
	virtual ~Merger() {}
	virtual bool open(std::string& err) = 0; // called once, and only when a path of two or more nodes has to be merged
	virtual bool set_contigs(const std::string& bytes, const std::vector<uint64_t>& offsets, std::string& err) = 0;
	virtual bool merge(uint32_t k, const std::vector<uint64_t>& noff, const std::vector<Node>& nodes, const std::vector<uint32_t>& ov, int verbose,
	    std::vector<uint64_t>& soff, const uint8_t*& seqs, std::vector<uint64_t>& acgt, std::vector<uint64_t>& loff, const char*& logs, std::string& err) = 0;
};

// main's option loop, MergeContigs.cpp:437-519.  Returns false when the caller should exit with `*status`.
inline bool parse_options(int argc, char** argv, Options& o, int* status)
{
	o.commandLine = cli::command_line(argc, argv);
	enum { OPT_HELP = 1, OPT_VERSION, OPT_DB, OPT_LIBRARY, OPT_STRAIN, OPT_SPECIES };
	static int format = DOT, onlyMerged = 0;
	static const struct option longopts[] = {
		{ "adj", no_argument, &format, ADJ }, { "dot", no_argument, &format, DOT }, { "dot-meancov", no_argument, &format, DOT_MEANCOV },
		{ "gfa", no_argument, &format, GFA1 }, { "gfa1", no_argument, &format, GFA1 }, { "gfa2", no_argument, &format, GFA2 },
		{ "gv", no_argument, &format, DOT }, { "sam", no_argument, &format, SAM },
		{ "graph", required_argument, NULL, 'g' }, { "kmer", required_argument, NULL, 'k' }, { "merged", no_argument, &onlyMerged, 1 },
		{ "out", required_argument, NULL, 'o' }, { "path", required_argument, NULL, 'p' }, { "verbose", no_argument, NULL, 'v' },
		{ "help", no_argument, NULL, OPT_HELP }, { "version", no_argument, NULL, OPT_VERSION },
		{ "db", required_argument, NULL, OPT_DB }, { "library", required_argument, NULL, OPT_LIBRARY },
		{ "strain", required_argument, NULL, OPT_STRAIN }, { "species", required_argument, NULL, OPT_SPECIES },
		{ NULL, 0, NULL, 0 }
	};
	bool die = false;
	std::string ignored;
	for (int c; (c = getopt_long(argc, argv, "g:k:o:v", longopts, NULL)) != -1;) {
		std::istringstream arg(optarg != NULL ? optarg : "");
		switch (c) {
		case '?': die = true; break;
		case 'g': arg >> o.graphPath; break;
		case 'k': arg >> o.k; break;
		case 'o': arg >> o.out; break;
		case 'v': o.verbose++; break;
		case OPT_HELP: fputs(USAGE_MESSAGE, stdout); *status = EXIT_SUCCESS; return false;
		case OPT_VERSION: fputs(VERSION_MESSAGE, stdout); *status = EXIT_SUCCESS; return false;
		case OPT_DB: case OPT_LIBRARY: case OPT_STRAIN: case OPT_SPECIES: arg >> ignored; break; // (this build keeps no database)
		} // (--path is in the reference's table and in no case of its switch: its argument is never read, so it is never at its end)
		if (optarg != NULL && !arg.eof()) {
			*status = cli::invalid_option(ABG_MC_PROGRAM, c, optarg);
			return false;
		}
	}
	o.format = format; o.onlyMerged = onlyMerged;
	if (o.k <= 0) { fprintf(stderr, ABG_MC_PROGRAM ": missing -k,--kmer option\n"); die = true; }
	if (o.out.empty()) { fprintf(stderr, ABG_MC_PROGRAM ": missing -o,--out option\n"); die = true; }
	if (argc - optind < 2) { fprintf(stderr, ABG_MC_PROGRAM ": missing arguments\n"); die = true; }
	if (argc - optind > 3) { fprintf(stderr, ABG_MC_PROGRAM ": too many arguments\n"); die = true; }
	if (die) {
		cli::try_help(ABG_MC_PROGRAM);
		*status = EXIT_FAILURE;
		return false;
	}
	o.contigPath = argv[optind++];
	if (argc - optind > 1) o.adjPath = argv[optind++];
	o.pathPath = argv[optind++];
	return true;
}

[[noreturn]] inline void fail(const std::string& msg) { cli::fail(ABG_MC_PROGRAM, msg); }

inline bool is_acgt(char c) { return strchr("ACGTacgt", c) != nullptr && c != 0; } // isACGT, Sequence.h:21-25

// Histogram (Common/Histogram.h) as far as printContiguityStats reads it
struct LengthHistogram {
	std::map<int, size_t> h;
	void insert(int x) { h[x]++; }
	typedef unsigned long long acc;
	size_t size() const { size_t n = 0; for (auto& e : h) n += e.second; return n; }
	acc sum() const { acc t = 0; for (auto& e : h) t += (acc)e.first * e.second; return t; }
	int minimum() const { return h.empty() ? 0 : h.begin()->first; }
	int maximum() const { return h.empty() ? 0 : h.rbegin()->first; }
	size_t count_from(int lo) const { size_t n = 0; for (auto it = h.lower_bound(lo); it != h.end(); ++it) n += it->second; return n; }
	int arg_min(acc x) const
	{
		acc t = 0;
		for (auto& e : h) { t += (acc)e.first * e.second; if (t >= x) return e.first; }
		return maximum();
	}
	int weighted_percentile(float p) const { return arg_min((acc)ceil(p * sum())); }
	double expected_value() const
	{
		double v = 0;
		const acc a = sum();
		for (auto& e : h) v += (double)e.first * e.first * e.second / a;
		return v;
	}
	LengthHistogram trim_low(int threshold) const
	{
		LengthHistogram r;
		for (auto& e : h) if (e.first >= threshold) r.h[e.first] += e.second;
		return r;
	}
};
template <class T> inline std::string to_eng(T n) // toEng, StringUtil.h:122-136
{
	std::ostringstream s;
	s << std::setprecision(4);
	if (n < 10000000) s << n;
	else if (n < 1e9) s << n / 1e6 << "e6";
	else if (n < 1e12) s << n / 1e9 << "e9";
	else s << n / 1e12 << "e12";
	return s.str();
}
inline std::string contiguity_stats(const LengthHistogram& h0, unsigned minSize) // printContiguityStats, Histogram.h:320-374
{
	const LengthHistogram h = h0.trim_low((int)minSize);
	std::ostringstream out;
	out << "n\tn:" << minSize << "\tL50\tmin\tN75\tN50\tN25\tE-size\tmax\tsum\tname\n";
	const unsigned n50 = (unsigned)h.weighted_percentile(0.5);
	out << to_eng(h0.size()) << '\t' << to_eng(h.size()) << '\t' << to_eng(h.count_from((int)n50)) << '\t';
	const unsigned long long sum = h.sum();
	out << to_eng(h.minimum()) << '\t' << to_eng(h.weighted_percentile(1 - 0.75)) << '\t' << to_eng(n50) << '\t' << to_eng(h.weighted_percentile(1 - 0.25)) << '\t'
	    << to_eng((unsigned)h.expected_value()) << '\t' << to_eng(h.maximum()) << '\t' << to_eng(sum);
	return out.str();
}

struct Contig { std::string comment, seq; };

class Run {
  public:
	Run(Options& o, Merger& m) : opt(o), merger(m) {}
	Options& opt;
	Merger& merger;
	cg::Graph graph;
	std::vector<Contig> contigs;
	std::vector<std::string> pathIDs;
	std::vector<Path> paths;
	int precision = 6; // of the floats written to stderr

	std::string name(Node u) const { return cg::node_name(graph, u); }
	std::string show(const Path& p) const { return cg::show_path(graph, p); }

	void read_contigs()
	{
		abghost::ReaderOptions ro; // FastaReader::NO_FOLD_CASE, opt::trimMasked = false (MergeContigs.cpp:437, 557)
		ro.foldCase = 0;
		ro.trimMasked = 0;
		abghost::FastaReader in(opt.contigPath, ro);
		std::string id, comment, s;
		unsigned count = 0;
		while (in.read(id, comment, s)) {
			if (!opt.adjPath.empty() && graph.index.count(id) == 0) continue;
			if (opt.adjPath.empty()) {
				const V u = graph.add_vertex((unsigned)s.size(), 0);
				graph.put_name(u, id);
			}
			if (graph.find_contig(id) != contigs.size())
				fail("`" + opt.contigPath + "': contig `" + id + "' is record " + std::to_string(contigs.size()) + " here and vertex " +
				    std::to_string(graph.find_contig(id)) + " of the graph: the two must be in the same order");
			contigs.push_back(Contig{ comment, s });
			++count;
		}
		if (opt.verbose > 0) fprintf(stderr, "Read %u sequences.\n", count);
		if (contigs.empty()) fail("`" + opt.contigPath + "' holds no contigs");
		if (!contigs[0].seq.empty() && isdigit((unsigned char)contigs[0].seq[0])) fail("`" + opt.contigPath + "' is in colour space, which this build does not read");
	}

	// find_vertex(name, g_contigNames), ContigNode.h:294-304
	Node find_node(std::string s) const
	{
		const std::string whole = s;
		const char c = s[s.size() - 1];
		s.erase(s.size() - 1);
		if (c != '+' && c != '-' && c != 'N') fail("`" + opt.pathPath + "': `" + whole + "' is no node: a node ends in +, - or N");
		if (c == 'N') {
			const unsigned long n = strtoul(s.c_str(), NULL, 0);
			if (n == 0 || n > 0x7fffffffUL) fail("`" + opt.pathPath + "': `" + whole + "' is no node: the gap must be positive");
			return -(Node)n;
		}
		return (Node)(2 * graph.find_contig(s) + (c == '-'));
	}

	// readPaths, MergeContigs.cpp:321-359 with operator>>(istream&, ContigPath&)
	void read_paths()
	{
		std::ifstream fin(opt.pathPath.c_str());
		if (opt.verbose > 0) fprintf(stderr, "Reading `%s'...\n", opt.pathPath.c_str());
		if (opt.pathPath != "-" && !fin.good()) { fprintf(stderr, "error: `%s': %s\n", opt.pathPath.c_str(), strerror(errno)); exit(EXIT_FAILURE); }
		std::istream& in = opt.pathPath == "-" ? std::cin : fin;
		unsigned count = 0;
		std::string id, line;
		while (in >> id && getline(in, line)) {
			Path path;
			std::istringstream ss(line);
			for (std::string n; ss >> n;) path.push_back(find_node(n));
			paths.push_back(path);
			pathIDs.push_back(id);
			++count;
		}
		if (opt.verbose > 0) fprintf(stderr, "Read %u paths.\n", count);
	}

	// sequence(contigs, id) of a path of one node, MergeContigs.cpp:159-171
	std::string sequence(Node u) const
	{
		if (u < 0) {
			const size_t n = (size_t)(-(int64_t)u);
			return std::string(opt.k - 1, 'N') + std::string(n, n < opt.k ? 'n' : 'N');
		}
		const std::string& s = contigs[(size_t)u >> 1].seq;
		return (u & 1) ? cg::reverse_complement(s) : s;
	}

	// get(vertex_bundle, g, u), MergeContigs.cpp:206-210
	void bundle(Node u, unsigned& l, unsigned& c) const
	{
		if (u < 0) { l = (unsigned)(-(int64_t)u) + opt.k - 1; c = 0; }
		else { l = graph.length[u]; c = graph.coverage[u]; }
	}
	int distance(Node u, Node v) const { return (u < 0 || v < 0) ? -(int)opt.k + 1 : graph.find_edge((V)u, (V)v)->d; }

	// outputGraph, MergeContigs.cpp:388-432
	void output_graph()
	{
		for (size_t i = 0; i < paths.size(); ++i) {
			const Path& path = paths[i];
			if (path.empty()) continue;
			unsigned l, c; // addProp, ContigGraphAlgorithms.h:146-160
			bundle(path[0], l, c);
			for (size_t j = 1; j < path.size(); ++j) {
				unsigned vl, vc;
				bundle(path[j], vl, vc);
				l += (unsigned)distance(path[j - 1], path[j]);
				l += vl;
				c += vc;
			}
			if (path.front() < 0 || path.back() < 0) fail("path `" + pathIDs[i] + "' begins or ends with a gap, which has no place in the graph");
			const V u = graph.add_vertex(l, c);
			cg::copy_out_edges(graph, (V)path.front() ^ 1, u ^ 1); // copy_in_edges
			cg::copy_out_edges(graph, (V)path.back(), u);
			graph.put_name(u, pathIDs[i]);
		}
		for (size_t i = 0; i < paths.size(); ++i) {
			const Path& path = paths[i];
			if (path.empty()) graph.remove_vertex(2 * graph.find_contig(pathIDs[i]));
			else {
				for (Node u : path) if (u >= 0) graph.clear_vertex((V)u);
				for (Node u : path) if (u >= 0) graph.remove_vertex((V)u);
			}
		}
		if (opt.verbose > 0) fprintf(stderr, "Writing `%s'...\n", opt.graphPath.c_str());
		FILE* g = fopen(opt.graphPath.c_str(), "wb");
		if (!g) { fflush(stdout); fprintf(stderr, "error: `%s': %s\n", opt.graphPath.c_str(), strerror(errno)); exit(EXIT_FAILURE); }
		{
			abgio::Out o(g);
			if (opt.format == DOT_MEANCOV) write_dot_meancov(o);
			else abgio::write_graph(o, graph, opt.format, ABG_MC_PROGRAM, opt.commandLine);
		}
		if (fclose(g) != 0) { fflush(stdout); fprintf(stderr, "error: `%s': %s\n", opt.graphPath.c_str(), strerror(errno)); exit(EXIT_FAILURE); }
		if (opt.verbose > 0) { cg::print_graph_stats(stderr, graph); precision = 2; } // (printGraphStats leaves cerr at setprecision(2), GraphUtil.h:56-63)
	}
	// dot_writer with the vertex property as opt::format == DOT_MEANCOV prints it (ContigProperties.h:86-99)
	void write_dot_meancov(abgio::Out& out) const
	{
		const int def = -(int)(opt.k - 1);
		out << "digraph adj {\n" << "graph [k=" << opt.k << "]\nedge [d=" << def << "]\n";
		for (uint64_t u = 0; u < graph.nv(); u++) {
			if (graph.removed(u)) continue;
			out << '"' << graph.vname((V)u) << "\" [l=" << graph.len(u) << " c=" << show_float((float)graph.cov(u) / (graph.len(u) - opt.k + 1)) << "]\n";
		}
		for (uint64_t u = 0; u < graph.nv(); u++) {
			if (graph.removed(u)) continue;
			graph.for_out(u, [&](uint32_t v, int d) {
				out << '"' << graph.vname((V)u) << "\" -> \"" << graph.vname(v) << '"';
				if (d != def) out << " [d=" << d << ']';
				out << '\n';
			});
		}
		out << "}\n";
	}

	int run()
	{
		if (!opt.adjPath.empty()) {
			if (opt.verbose > 0) fprintf(stderr, "Reading `%s'...\n", opt.adjPath.c_str());
			cg::load_graph(opt.adjPath, opt.k, graph, fail);
			if (opt.verbose > 0) fprintf(stderr, "Read %llu vertices.\n", (unsigned long long)graph.nv());
		}
		graph.k = opt.k;
		if (opt.verbose > 0) fprintf(stderr, "Reading `%s'...\n", opt.contigPath.c_str());
		read_contigs();
		read_paths();

		// seenContigs and markRemovedContigs, MergeContigs.cpp:361-385
		std::vector<bool> seen(contigs.size());
		for (const Path& p : paths)
			for (Node u : p) if (u >= 0 && ((size_t)u >> 1) < seen.size()) seen[(size_t)u >> 1] = true;
		for (size_t i = 0; i < paths.size(); ++i)
			if (paths[i].empty()) {
				const unsigned id = graph.find_contig(pathIDs[i]);
				if (id >= seen.size()) fail("`" + opt.pathPath + "': `" + pathIDs[i] + "' is to be removed and `" + opt.contigPath + "' does not hold it");
				seen[id] = true;
			}

		LengthHistogram lengths;
		FILE* out = opt.out == "-" ? stdout : fopen(opt.out.c_str(), "wb");
		if (!out) { fprintf(stderr, "error: `%s': %s\n", opt.out.c_str(), strerror(errno)); return EXIT_FAILURE; }
		if (!opt.onlyMerged)
			for (size_t i = 0; i < contigs.size(); ++i) {
				if (seen[i]) continue;
				const Contig& c = contigs[i];
				fprintf(out, ">%s", graph.names[i].c_str());
				if (!c.comment.empty()) fprintf(out, " %s", c.comment.c_str());
				fputc('\n', out);
				fwrite(c.seq.data(), 1, c.seq.size(), out);
				fputc('\n', out);
				if (opt.verbose > 0) lengths.insert((int)std::count_if(c.seq.begin(), c.seq.end(), is_acgt));
			}

		// every junction of every path of two or more nodes, up to the first one the reference asserts on
		std::vector<uint64_t> noff{ 0 };
		std::vector<Node> nodes;
		std::vector<uint32_t> ov;
		std::vector<size_t> slot(paths.size(), SIZE_MAX);
		size_t stop = paths.size();
		std::string stop_line, stop_msg;
		for (size_t i = 0; i < paths.size() && stop == paths.size(); ++i) {
			const Path& p = paths[i];
			if (p.size() < 2) {
				if (p.size() == 1 && p[0] >= 0 && ((size_t)p[0] >> 1) >= contigs.size()) { stop = i; stop_msg = "`" + opt.contigPath + "' does not hold contig `" + graph.names[(size_t)p[0] >> 1] + "' of path `" + pathIDs[i] + "'"; }
				continue;
			}
			for (size_t j = 0; j < p.size() && stop == paths.size(); ++j) {
				uint32_t o = 0;
				if (p[j] >= 0 && ((size_t)p[j] >> 1) >= contigs.size()) { stop = i; stop_msg = "`" + opt.contigPath + "' does not hold contig `" + graph.names[(size_t)p[j] >> 1] + "' of path `" + pathIDs[i] + "'"; break; }
				if (j > 0) {
					int d = -(int)opt.k + 1;
					if (p[j - 1] >= 0 && p[j] >= 0) {
						const cg::Edge* e = graph.find_edge((V)p[j - 1], (V)p[j]);
						if (!e) {
							stop = i;
							stop_line = "error: no edge " + name(p[j - 1]) + " -> " + name(p[j]) + "\n";
							stop_msg = "path `" + pathIDs[i] + "' of `" + opt.pathPath + "' takes an edge the graph lacks";
							break;
						}
						d = e->d;
					}
					if (d >= 0) {
						stop = i;
						stop_msg = "path `" + pathIDs[i] + "' of `" + opt.pathPath + "': the edge " + name(p[j - 1]) + " -> " + name(p[j]) + " has distance " + std::to_string(d) + ", and only overlapping contigs can be merged";
						break;
					}
					o = (uint32_t)-d;
				}
				nodes.push_back(p[j]);
				ov.push_back(o);
			}
			if (stop != paths.size()) { nodes.resize(noff.back()); ov.resize(noff.back()); break; }
			slot[i] = noff.size() - 1;
			noff.push_back(nodes.size());
		}

		std::vector<uint64_t> soff{ 0 }, acgt, loff{ 0 };
		const uint8_t* seqs = nullptr;
		const char* logs = nullptr;
		if (noff.size() > 1) {
			std::string err;
			if (!merger.open(err)) fail(err);
			std::string bytes;
			std::vector<uint64_t> offsets;
			cg::flatten(contigs, [](const Contig& c) -> const std::string& { return c.seq; }, bytes, offsets);
			if (!merger.set_contigs(bytes, offsets, err)) fail(err);
			if (!merger.merge(opt.k, noff, nodes, ov, opt.verbose, soff, seqs, acgt, loff, logs, err)) fail(err);
		}

		unsigned npaths = 0;
		std::string header;
		for (size_t i = 0; i < stop; ++i) {
			const Path& p = paths[i];
			if (p.empty()) continue;
			unsigned coverage = 0;
			for (Node u : p) if (u >= 0) coverage += graph.coverage[u];
			std::string single;
			const uint8_t* seq;
			size_t len, count;
			if (p.size() == 1) {
				single = sequence(p[0]);
				seq = (const uint8_t*)single.data();
				len = single.size();
				count = opt.verbose > 0 ? (size_t)std::count_if(single.begin(), single.end(), is_acgt) : 0;
			} else {
				const size_t q = slot[i];
				seq = seqs + soff[q];
				len = soff[q + 1] - soff[q];
				count = acgt[q];
				if (loff[q + 1] > loff[q]) { // the names into what the merger logged
					std::string text;
					for (uint64_t x = loff[q]; x < loff[q + 1]; ++x) {
						if (logs[x] == '\x01') {
							size_t j = 0;
							for (++x; logs[x] != '\x02'; ++x) j = j * 10 + (logs[x] - '0');
							text += name(p[j]);
						} else if (logs[x] == '\x03') text += show(p);
						else text += logs[x];
					}
					fflush(out);
					fputs(text.c_str(), stderr);
				}
			}
			// pathToComment, MergeContigs.cpp:280-291
			header = ">" + pathIDs[i] + " " + std::to_string(len) + " " + std::to_string(coverage) + " " + name(p.front());
			if (p.size() == 3) header += "," + name(p[1]);
			else if (p.size() > 3) header += ",...";
			if (p.size() > 1) header += "," + name(p.back());
			header += '\n';
			fwrite(header.data(), 1, header.size(), out);
			fwrite(seq, 1, len, out);
			fputc('\n', out);
			npaths++;
			if (opt.verbose > 0) lengths.insert((int)count);
		}
		if (stop != paths.size()) {
			fflush(out);
			fputs(stop_line.c_str(), stderr);
			fail(stop_msg);
		}
		if (fflush(out) != 0 || ferror(out)) { fprintf(stderr, "error: `%s': %s\n", opt.out.c_str(), strerror(errno)); return EXIT_FAILURE; }

		if (!opt.graphPath.empty()) output_graph();
		if (npaths == 0) return 0;

		float minCov = std::numeric_limits<float>::infinity(), minCovUsed = std::numeric_limits<float>::infinity();
		for (size_t i = 0; i < contigs.size(); i++) {
			const unsigned cov = graph.coverage[2 * i], len = graph.length[2 * i];
			if (cov == 0 || len < opt.k) continue;
			const float c = (float)cov / (len - opt.k + 1);
			minCov = std::min(minCov, c);
			if (seen[i]) minCovUsed = std::min(minCovUsed, c);
		}
		fprintf(stderr, "The minimum coverage of single-end contigs is %s.\nThe minimum coverage of merged contigs is %s.\n", show_float(minCov, precision).c_str(),
		    show_float(minCovUsed, precision).c_str());
		if (minCov < minCovUsed) fprintf(stderr, "Consider increasing the coverage threshold parameter, c, to %s.\n", show_float(minCovUsed, precision).c_str());
		if (opt.verbose > 0) fprintf(stderr, "%s\t%s\n", contiguity_stats(lengths, 200).c_str(), opt.out.c_str());
		if (out != stdout && fclose(out) != 0) { fprintf(stderr, "error: `%s': %s\n", opt.out.c_str(), strerror(errno)); return EXIT_FAILURE; }
		return 0;
	}
};

inline int run_main(int argc, char** argv, Merger& m)
{
	Options o;
	int status = 0;
	if (!parse_options(argc, argv, o, &status)) return status;
	Run r(o, m);
	return r.run();
}

} // namespace mc
