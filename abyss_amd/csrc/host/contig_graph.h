// contig_graph.h -- the contig graph of the drop-in binaries that take one (abyss-rresolver-short, Overlap, SimpleGraph, MergeContigs,
// PopBubbles): the graph with its dictionary of names, its readers for the GraphViz and ADJ formats, the loader around them, and the
// few things about contigs and their paths that more than one of those binaries writes.  Nothing here knows a program's options.
//
// Reference behaviour restated here (ABySS 2.3.10):
//   Graph/DirectedGraph.h, ContigGraph.h     adjacency lists in insertion order; (u,v) implies (~v,~u)
//   Graph/ContigGraphAlgorithms.h:40-87      contiguous_out/in, copy_out_edges
//   Graph/DotIO.h:150-309, AdjIO.h:99-190    readers;  Common/ContigID.h, Dictionary.h  contig names
//   Common/ContigNode.h:41-48,215-232, ContigPath.h:37-45   the <n>N node and the path writer
// What the graph and its readers say on stderr names no program (`error: ...'), so it reads the same from all five; what
// load_graph itself refuses goes through the caller's fail.
#pragma once

#include "graph_writers.h"

#include <algorithm>
#include <cctype>
#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <unordered_map>
#include <vector>

namespace cg {

[[noreturn]] inline void die(const std::string& msg)
{
	fprintf(stderr, "%s\n", msg.c_str());
	exit(EXIT_FAILURE);
}

// ---- the contig graph: ContigGraph<DirectedGraph<ContigProperties, Distance>> + g_contigNames -------------------------
typedef uint32_t V; // vertex = 2 * contig + sense (ContigNode)
struct Edge { V v; int d; };

struct Graph {
	unsigned k = 0;
	std::vector<std::vector<Edge>> adj; // out-edges in insertion order
	std::vector<unsigned> length, coverage; // per VERTEX (the reference keeps a copy of the properties on both)
	std::vector<bool> rem;
	// g_contigNames + g_nextContigName (Common/ContigID.h, Dictionary.h)
	std::vector<std::string> names;
	std::unordered_map<std::string, unsigned> index;
	unsigned nextName = 0;

	uint64_t nv() const { return adj.size(); }
	bool removed(uint64_t u) const { return u < rem.size() && rem[u]; }
	const std::string& cname(uint64_t u) const { return names[u >> 1]; }
	unsigned len(uint64_t u) const { return length[u]; }
	unsigned cov(uint64_t u) const { return coverage[u]; }
	template <class F> void for_out(uint64_t u, F f) const { for (const Edge& e : adj[u]) f(e.v, e.d); }
	std::string vname(V u) const { return names[u >> 1] + ((u & 1) ? '-' : '+'); }

	// Dictionary::put (Dictionary.h:48-60) through put(vertex_name, ...) (ContigNode.h:236-247)
	void put_name(V u, std::string name)
	{
		const char c = name.empty() ? 0 : name[name.size() - 1];
		if (c == '+' || c == '-') name.erase(name.size() - 1);
		const unsigned id = u >> 1;
		if (id < names.size()) {
			if (names[id] != name) die("error: the names of vertex " + std::to_string(u) + " do not agree: `" + names[id] + "', `" + name + "'");
			return;
		}
		if (id != names.size()) die("error: vertices out of order near `" + name + "'");
		if (!index.emplace(name, id).second) { fprintf(stderr, "error: duplicate ID: `%s'\n", name.c_str()); exit(EXIT_FAILURE); }
		names.push_back(name);
	}
	// find_vertex (ContigNode.h:283-303)
	V find_vertex(std::string name) const
	{
		if (name.size() < 2) die("error: unexpected ID: `" + name + "'");
		const char c = name[name.size() - 1];
		name.erase(name.size() - 1);
		if (c != '+' && c != '-') die("error: unexpected ID: `" + name + c + "'");
		return find_contig(name) * 2 + (c == '-');
	}
	unsigned find_contig(const std::string& name) const
	{
		auto it = index.find(name);
		if (it == index.end()) { fprintf(stderr, "error: unexpected ID: `%s'\n", name.c_str()); exit(EXIT_FAILURE); }
		return it->second;
	}
	// createContigName / setNextContigName (ContigID.h:31-61)
	std::string create_name()
	{
		if (nextName == 0) {
			unsigned mx = 0;
			for (const std::string& s : names) {
				std::istringstream iss(s);
				unsigned x;
				if (iss >> x && iss.eof() && x > mx) mx = x;
			}
			nextName = names.empty() ? 0 : 1 + mx;
		}
		return std::to_string(nextName++);
	}

	// DirectedGraph
	V add_vertex1(unsigned l, unsigned c) { adj.emplace_back(); length.push_back(l); coverage.push_back(c); return (V)(adj.size() - 1); }
	void add_edge1(V u, V v, int d) { adj[u].push_back(Edge{ v, d }); }
	void remove_edge1(V u, V v)
	{
		auto& e = adj[u];
		e.erase(std::remove_if(e.begin(), e.end(), [v](const Edge& x) { return x.v == v; }), e.end());
	}
	const Edge* find_edge(V u, V v) const
	{
		for (const Edge& e : adj[u]) if (e.v == v) return &e;
		return nullptr;
	}
	bool has_edge(V u, V v) const { return find_edge(u, v) != nullptr; }
	// get(edge_bundle, g, u, v) (ContigProperties.h:187-205)
	int dist(V u, V v) const
	{
		const Edge* e = find_edge(u, v);
		if (!e) die("error: no edge " + vname(u) + " -> " + vname(v));
		return e->d;
	}
	unsigned out_degree(V u) const { return (unsigned)adj[u].size(); }
	uint64_t num_edges() const { uint64_t n = 0; for (auto& a : adj) n += a.size(); return n; }
	// ContigGraph (ContigGraph.h:124-228)
	unsigned in_degree(V u) const { return (unsigned)adj[u ^ 1].size(); }
	V add_vertex(unsigned l, unsigned c) { const V v = add_vertex1(l, c); add_vertex1(l, c); return v; }
	void add_edge(V u, V v, int d) { add_edge1(u, v, d); if (u != (v ^ 1)) add_edge1(v ^ 1, u ^ 1, d); }
	void remove_edge(V u, V v) { remove_edge1(u, v); if (u != (v ^ 1)) remove_edge1(v ^ 1, u ^ 1); }
	void clear_out_edges(V u)
	{
		for (const Edge& e : adj[u]) if ((e.v ^ 1) != u) remove_edge1(e.v ^ 1, u ^ 1);
		adj[u].clear();
	}
	void clear_vertex(V v) { clear_out_edges(v); clear_out_edges(v ^ 1); }
	void remove_vertex(V v)
	{
		if (rem.size() < adj.size()) rem.resize(adj.size(), false);
		rem[v] = true;
		rem[v ^ 1] = true;
	}
	uint64_t num_removed() const { uint64_t n = 0; for (uint64_t u = 0; u < nv(); u++) n += removed(u); return n; }
};

inline void print_graph_stats(FILE* out, const Graph& g)
{
	std::map<int, uint64_t> h;
	for (uint64_t u = 0; u < g.nv(); u++) if (!g.removed(u)) h[(int)g.out_degree((V)u)]++;
	abgio::print_graph_stats(out, (unsigned)(g.nv() - g.num_removed()), (unsigned)g.num_edges(), h);
}

// ---- readers ---------------------------------------------------------------------------------------------------
// A cursor over the whole file with the stream manipulators the reference parses with (Common/IOUtil.h:38-84)
struct Cursor {
	const std::string& s;
	size_t p = 0;
	explicit Cursor(const std::string& s) : s(s) {}
	bool eof() const { return p >= s.size(); }
	int peek() const { return eof() ? EOF : (unsigned char)s[p]; }
	void ws() { while (!eof() && isspace((unsigned char)s[p])) p++; }
	void expect(const char* pat) // operator>>(istream&, expect)
	{
		for (const char* q = pat; *q; ++q) {
			if (*q == ' ') { ws(); continue; }
			if (eof() || s[p] != *q) {
				fprintf(stderr, "error: Expected `%s' and saw ", q);
				if (eof()) fprintf(stderr, "end-of-file\n");
				else {
					const size_t e = s.find('\n', p);
					fprintf(stderr, "`%c'\nnear: %s\n", s[p], s.substr(p, e == std::string::npos ? e : e - p).c_str());
				}
				exit(EXIT_FAILURE);
			}
			p++;
		}
	}
	void ignore(char delim) { const size_t e = s.find(delim, p); p = e == std::string::npos ? s.size() : e + 1; }
	bool number(long long& x) // operator>>(int): leading whitespace, sign, digits
	{
		ws();
		size_t q = p;
		if (q < s.size() && (s[q] == '-' || s[q] == '+')) q++;
		if (q >= s.size() || !isdigit((unsigned char)s[q])) return false;
		x = strtoll(s.c_str() + p, nullptr, 10);
		while (q < s.size() && isdigit((unsigned char)s[q])) q++;
		p = q;
		return true;
	}
	unsigned uns(const char* what) { long long x; if (!number(x) || x < 0) die(std::string("error: expected a number (") + what + ")"); return (unsigned)x; }
	int integer(const char* what) { long long x; if (!number(x)) die(std::string("error: expected a number (") + what + ")"); return (int)x; }
	bool quoted(std::string& out) // read_dot_name
	{
		ws();
		if (peek() != '"') return false;
		p++;
		const size_t e = s.find('"', p);
		out = s.substr(p, e == std::string::npos ? e : e - p);
		p = e == std::string::npos ? s.size() : e + 1;
		return true;
	}
};
// operator>>(istream&, ContigProperties&) (ContigProperties.h:112-126) and Distance (:160-168)
inline void read_props(Cursor& in, unsigned& l, unsigned& c)
{
	in.ws();
	if (in.peek() == 'l') {
		in.expect("l =");
		l = in.uns("l");
		in.ws();
		if (in.peek() == 'C') { in.expect("C ="); c = in.uns("C"); }
	} else if (in.peek() == 'C') {
		in.expect("C=");
		c = in.uns("C");
		in.expect(", l=");
		l = in.uns("l");
	} else {
		l = in.uns("length");
		c = in.uns("coverage");
	}
}
inline int read_distance(Cursor& in)
{
	in.expect(" d = ");
	if (in.peek() == '"') { in.expect("\""); const int d = in.integer("d"); in.expect("\""); return d; }
	return in.integer("d");
}

// read_dot (Graph/DotIO.h:150-309) on the plain directed graph: every line of the file is one vertex or one edge.  k is the k-mer
// size the caller expects (0: whatever the file says); a file that names another one ends the run, so k leaves as it came unless
// it came as 0.
inline void read_dot(const std::string& text, Graph& g, unsigned& k)
{
	Cursor in(text);
	in.ws();
	in.expect("digraph");
	in.ignore('{');
	int defd = -(int)k + 1;
	for (bool done = false; !done;) {
		in.ws();
		if (in.eof()) break;
		switch (in.peek()) {
		case 'g':
			in.expect("graph [ ");
			if (in.peek() == 'k') {
				in.expect("k =");
				const unsigned fk = in.uns("k");
				if (k > 0 && fk != k) die("error: the graph was built with k=" + std::to_string(fk) + ", not " + std::to_string(k));
				k = fk;
				defd = -(int)k + 1;
			}
			in.ignore(']');
			break;
		case 'e':
			in.expect("edge [");
			defd = read_distance(in);
			in.ignore(']');
			break;
		default: done = true; break;
		}
		in.ws();
		if (in.peek() == ';') in.p++;
	}
	const bool addVertices = g.nv() == 0;
	for (std::string uname; in.quoted(uname);) {
		in.ws();
		if (in.eof()) die("error: unexpected end of the graph file");
		const char c = in.s[in.p++];
		if (c == ';' || c == '[') {
			unsigned l = 0, cv = 0;
			if (c == '[') { read_props(in, l, cv); in.ignore(']'); }
			if (addVertices) { const V u = g.add_vertex1(l, cv); g.put_name(u, uname); }
			else {
				const V u = g.find_vertex(uname);
				if (c == '[' && (g.length[u] != l || g.coverage[u] != cv)) die("error: vertex properties do not agree: \"" + uname + "\"");
			}
		} else if (c == '-') {
			in.expect(">");
			const V u = g.find_vertex(uname);
			in.ws();
			if (in.peek() == '{') {
				in.expect("{");
				for (std::string vn; in.quoted(vn);) g.add_edge1(u, g.find_vertex(vn), defd);
				in.expect(" }");
			} else {
				std::string vn;
				if (!in.quoted(vn)) { fprintf(stderr, "error: Expected `\"' and saw `%c'.\n", (char)in.peek()); exit(EXIT_FAILURE); }
				const V v = g.find_vertex(vn);
				int d = defd;
				in.ws();
				if (in.peek() == '[') { in.expect("["); d = read_distance(in); in.ignore(']'); }
				if (g.has_edge(u, v)) { // DisallowParallelEdges, GraphIO.h:84-92
					fprintf(stderr, "error: parallel edges: [d=%d], [d=%d]\n", g.dist(u, v), d);
					exit(EXIT_FAILURE);
				}
				g.add_edge1(u, v, d);
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
	if (!in.eof()) die("error: Expected end-of-file after the graph");
	if (g.nv() == 0) die("error: the graph has no vertices");
}

// read_adj (Graph/AdjIO.h:99-190), ADJ format: "name length coverage\t; out-edges\t; in-edges"
inline void read_adj(const std::string& text, Graph& g, unsigned k)
{
	const int defd = -(int)k + 1;
	std::vector<std::pair<size_t, size_t>> lines; // [begin, end)
	for (size_t a = 0; a < text.size();) {
		size_t e = text.find('\n', a);
		if (e == std::string::npos) e = text.size();
		if (e > a) lines.push_back({ a, e });
		a = e + 1;
	}
	if (lines.empty()) die("error: the graph file is empty");
	{
		const std::string first = text.substr(lines[0].first, lines[0].second - lines[0].first);
		if (std::count(first.begin(), first.end(), ';') != 2) die("error: the graph is neither GraphViz nor ADJ format (the formats this build reads)");
	}
	for (auto& ln : lines) {
		std::istringstream ss(text.substr(ln.first, ln.second - ln.first));
		std::string name;
		unsigned l = 0, c = 0;
		if (!(ss >> name >> l >> c)) die("error: malformed ADJ line");
		const V u = g.add_vertex(l, c);
		g.put_name(u, name);
	}
	for (auto& ln : lines) {
		const std::string line = text.substr(ln.first, ln.second - ln.first);
		const size_t s1 = line.find(';'), s2 = line.find(';', s1 + 1);
		std::istringstream head(line.substr(0, s1));
		std::string name;
		head >> name;
		const V u = 2 * g.find_contig(name);
		for (unsigned sense = 0; sense < 2; sense++) {
			std::string part = sense == 0 ? line.substr(s1 + 1, s2 - s1 - 1) : line.substr(s2 + 1);
			Cursor in(part);
			for (;;) {
				in.ws();
				if (in.eof()) break;
				size_t e = in.p;
				while (e < part.size() && !isspace((unsigned char)part[e])) e++;
				const std::string vn = part.substr(in.p, e - in.p);
				in.p = e;
				in.ws();
				const V v = g.find_vertex(vn);
				int d = defd;
				if (in.peek() == '[') { in.p++; d = read_distance(in); in.ignore(']'); }
				if (g.has_edge(u ^ sense, v ^ sense)) die("error: parallel edges in the ADJ file near `" + vn + "'");
				g.add_edge1(u ^ sense, v ^ sense, d);
			}
		}
	}
}

inline std::string slurp(const std::string& path)
{
	std::ifstream f(path, std::ios::binary);
	if (!f.good()) { fprintf(stderr, "error: `%s': %s\n", path.c_str(), strerror(errno)); exit(EXIT_FAILURE); }
	std::ostringstream ss;
	ss << f.rdbuf();
	return ss.str();
}

// The graph file `path` into the empty graph g, in whichever of the two formats its first byte says it is.  fail(msg) gets what is
// wrong with the file as a whole, without a prefix, and does not return; what is wrong inside the file is the readers' to report.
// k is the program's -k and is written back, since read_dot takes the file's k when it is given 0.  All five programs refuse a
// missing or zero -k before they load, and read_dot ends the run when the file's k differs from a positive one, so the write-back
// never changes a value.
template <class Fail>
inline void load_graph(const std::string& path, unsigned& k, Graph& g, Fail fail)
{
	const std::string text = slurp(path);
	size_t p = 0;
	while (p < text.size() && isspace((unsigned char)text[p])) p++;
	const int c = p < text.size() ? text[p] : EOF;
	if (c == 'd') read_dot(text, g, k);
	else if (c == '@' || c == 'H' || c == '>' || c == 'g') // SAM, GFA, FASTA (ASQG has H too), an undirected GraphViz graph
		fail("`" + path + "': this build reads the contig graph in GraphViz (--dot) or ADJ format only");
	else read_adj(text, g, k);
	g.k = k;
	if (g.nv() & 1) fail("`" + path + "': a contig is missing one of its two vertices");
}

inline std::string reverse_complement(const std::string& s)
{
	std::string r(s.rbegin(), s.rend());
	for (auto& c : r) {
		switch (c) { // complementBaseChar, Common/Sequence.cpp:21-47
		case 'A': c = 'T'; break; case 'C': c = 'G'; break; case 'G': c = 'C'; break; case 'T': c = 'A'; break;
		case 'a': c = 't'; break; case 'c': c = 'g'; break; case 'g': c = 'c'; break; case 't': c = 'a'; break;
		case 'N': case 'n': case '.': break;
		case 'M': c = 'K'; break; case 'R': c = 'Y'; break; case 'W': case 'S': break; case 'Y': c = 'R'; break; case 'K': c = 'M'; break;
		case 'V': c = 'B'; break; case 'H': c = 'D'; break; case 'D': c = 'H'; break; case 'B': c = 'V'; break;
		default: fprintf(stderr, "error: unexpected character: `%c'\n", c); exit(EXIT_FAILURE);
		}
	}
	return r;
}

// contiguous_out, contiguous_in, copy_out_edges (ContigGraphAlgorithms.h:40-87); copy_in_edges is copy_out_edges of the complements
inline bool contiguous_out(const Graph& g, V u) { return g.out_degree(u) == 1 && g.in_degree(g.adj[u][0].v) == 1; }
inline bool contiguous_in(const Graph& g, V u) { return contiguous_out(g, u ^ 1); }
inline void copy_out_edges(Graph& g, V u, V uout)
{
	bool palindrome = false;
	int pd = 0;
	const size_t n = g.adj[u].size(); // (u's own list does not change in here)
	for (size_t i = 0; i < n; i++) {
		const Edge e = g.adj[u][i];
		if ((e.v ^ 1) == u) { palindrome = true; pd = e.d; }
		else g.add_edge(uout, e.v, e.d);
	}
	if (palindrome) { g.add_edge(uout, u ^ 1, pd); g.add_edge(uout, uout ^ 1, pd); }
}

// ---- paths and contigs as more than one program writes them -----------------------------------------------------------
typedef int32_t Node; // ContigNode: a vertex, or -n for the gap (the ambiguous node) of n bases (ContigNode.h:41-48)
typedef std::vector<Node> Path;

inline std::string node_name(const Graph& g, Node u) { return u < 0 ? std::to_string(-(int64_t)u) + "N" : g.vname((V)u); }
inline std::string show_path(const Graph& g, const Path& p) // operator<<(ostream&, const ContigPath&), ContigPath.h:37-45
{
	std::string s;
	for (size_t i = 0; i < p.size(); ++i) { if (i) s += ' '; s += node_name(g, p[i]); }
	return s;
}

inline std::string show_float(float x, int precision = 6) // operator<<(ostream&, float)
{
	char b[64];
	snprintf(b, sizeof b, "%.*g", precision, (double)x);
	return b;
}

// the contigs end to end and where each begins and the last ends, as the searchers' and the merger's set_contigs take them;
// seq(c) is the bases of a contig
template <class Contigs, class Seq>
inline void flatten(const Contigs& contigs, Seq seq, std::string& bytes, std::vector<uint64_t>& offsets)
{
	size_t total = 0;
	for (const auto& c : contigs) total += seq(c).size();
	bytes.clear();
	bytes.reserve(total);
	offsets.assign(1, 0);
	for (const auto& c : contigs) { bytes += seq(c); offsets.push_back(bytes.size()); }
}

} // namespace cg
