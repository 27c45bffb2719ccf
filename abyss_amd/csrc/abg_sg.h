// abg_sg.h -- the constrained path search of SimpleGraph (bin/abyss-pe:663-664): every path from one contig end through the overlap
// graph that meets the distance estimates of that end.
//
// Reference behaviour restated here (ABySS 2.3.10, paths relative to the repo):
//   Graph/ConstrainedSearch.h:56-119   the recursive search; :124-144 its entry (constraints sorted by vertex, then a copy by bound)
//   Graph/ConstrainedSearch.h:41-51    findConstraint: lower_bound on the vertex-sorted list, so of a vertex listed twice only the
//                                      first entry is ever found and the second can never be satisfied
//   Graph/ConstrainedSearch.h:16-21    maxCost 100000 (--max-cost), maxPaths 200
//   SimpleGraph/SimpleGraph.cpp:490-494  what the caller reads: numVisited >= maxCost and solutions.size() > maxPaths
//
// The recursion as a loop.  A call of the reference with a path that ends in v does one of four things: (a) v is an unsatisfied
// constraint whose bound the distance exceeds: return; (b) v satisfies the last open constraint: record the path, and stop the
// whole search once more than maxPaths are recorded (the extra one stays recorded); (c) v satisfies a constraint that is not the
// last: mark it and call itself again with the same path, which then falls through to (d), and unmark it on the way back; (d) count
// the visit (stop the whole search when the count reaches maxCost), return when some open constraint has a bound below the distance,
// else add v's length and try every out-edge of v in order.  Here a frame is what (d) leaves on the reference's stack: the vertex, the
// cursor into its out-edges, the distance after the vertex's length, and the constraint (c) marked on the way in (-1: none), which
// is unmarked when the frame is popped.  sg_step examines one out-edge of the top frame, or pops it.
//
// The nextConstraint walk (ConstrainedSearch.h:95-101) skips, in bound order, entries whose bound is below the distance and whose
// vertex looks satisfied, then returns when the next entry's bound is below the distance.  The skipped entries look satisfied and the
// one it stops at does not, so it returns exactly when some entry has bound < distance and a vertex that does not look satisfied:
// the order of equal bounds cannot matter, and no sorted copy is needed.  "Looks satisfied" goes through findConstraint, so for a
// vertex listed twice it is the state of its first entry.  Where every entry looks satisfied and all bounds are below the distance
// the reference walks off its list (undefined); that needs a vertex listed twice, finds no further solution, and goes on here
// without a prune.
//
// The graph is CSR over oriented vertices (2 * contig + sense): voff[nv + 1], vlen[nv], and per edge its target and distance in the
// order the reference's reader adds them, which is the order the search tries them in.  Constraints are sorted by (vertex, bound).
#pragma once
#include "abg_core.h"
#include <cstdint>

namespace abg {

struct SGGraph { const uint32_t* voff; const uint32_t* vlen; const uint32_t* etgt; const int32_t* edist; uint32_t nv; };
struct SGFrame { uint32_t u, cur; int32_t dist, csat; };
// what one search is given: its origin and where its constraints lie in the shared sorted arrays
struct SGJob { uint32_t origin, coff, nc, pad; };

enum { SG_RUNNING = 0, SG_DONE = 1, SG_ESTACK = 2, SG_EARENA = 3, SG_ECONSTRAINTS = 4 };

constexpr uint32_t SG_MAX_CONSTRAINTS = 64; // the device keeps the satisfied marks in one 64-bit word

struct SGSat64 {
	uint64_t m = 0;
	ABG_HD bool test(uint32_t i) const { return (m >> i) & 1; }
	ABG_HD void set(uint32_t i) { m |= 1ull << i; }
	ABG_HD void clear(uint32_t i) { m &= ~(1ull << i); }
	ABG_HD void reset() { m = 0; }
};

template <class Sat> struct SGState {
	SGFrame f;
	uint32_t depth, satisfied, visited, nsol;
	Sat sat;
};

// findConstraint: the first entry of vertex v, or -1
ABG_HD int32_t sg_find(const uint32_t* __restrict__ cv, uint32_t nc, uint32_t v)
{
	uint32_t lo = 0, hi = nc;
	while (lo < hi) {
		const uint32_t mid = (lo + hi) / 2;
		if (cv[mid] < v) lo = mid + 1; else hi = mid;
	}
	return lo < nc && cv[lo] == v ? (int32_t)lo : -1;
}

// is there an entry with bound < distance whose vertex does not look satisfied?
template <class Sat> ABG_HD bool sg_violated(const uint32_t* __restrict__ cv, const int32_t* __restrict__ cb, uint32_t nc, const Sat& sat, int32_t distance)
{
	uint32_t first = 0;
	for (uint32_t i = 0; i < nc; ++i) {
		if (i > 0 && cv[i] != cv[i - 1]) first = i;
		if (distance > cb[i] && !sat.test(first)) return true;
	}
	return false;
}

template <class Sat> ABG_HD void sg_begin(const SGGraph& g, uint32_t origin, SGState<Sat>& s)
{
	s.f.u = origin;
	s.f.cur = g.voff[origin];
	s.f.dist = 0;
	s.f.csat = -1;
	s.depth = s.satisfied = s.visited = s.nsol = 0;
	s.sat.reset();
}

// One step.  Stack: cap(), store(i, frame), load(i), vertex(i) for i < cap(); frames 0 .. depth - 1 are stored, s.f is the top.
// Sink: emit(stack, depth, top vertex, v) records the path vertex(1) .. vertex(depth - 1), top vertex (when depth > 0), v and
// returns false when it has no room.
template <class Sat, class Stack, class Sink>
ABG_HD int sg_step(const SGGraph& g, const uint32_t* __restrict__ cv, const int32_t* __restrict__ cb, uint32_t nc, uint32_t max_cost, uint32_t max_paths,
    SGState<Sat>& s, Stack& st, Sink& sink)
{
	if (s.f.cur == g.voff[s.f.u + 1]) { // every out-edge tried: back to the caller
		if (s.f.csat >= 0) { s.sat.clear((uint32_t)s.f.csat); --s.satisfied; }
		if (s.depth == 0) return SG_DONE;
		s.f = st.load(--s.depth);
		return SG_RUNNING;
	}
	const uint32_t e = s.f.cur++;
	const uint32_t v = g.etgt[e];
	const int32_t distance = s.f.dist + g.edist[e];
	int32_t csat = -1;
	const int32_t c = sg_find(cv, nc, v);
	if (c >= 0 && !s.sat.test((uint32_t)c)) {
		if (distance > cb[c]) return SG_RUNNING; // this constraint cannot be met
		if (s.satisfied + 1 == nc) {
			if (!sink.emit(st, s.depth, s.f.u, v)) return SG_EARENA;
			return ++s.nsol <= max_paths ? SG_RUNNING : SG_DONE;
		}
		s.sat.set((uint32_t)c);
		++s.satisfied;
		csat = c;
	}
	if (++s.visited >= max_cost) return SG_DONE; // too complex
	if (sg_violated(cv, cb, nc, s.sat, distance)) {
		if (csat >= 0) { s.sat.clear((uint32_t)csat); --s.satisfied; }
		return SG_RUNNING;
	}
	if (s.depth >= st.cap()) return SG_ESTACK;
	st.store(s.depth++, s.f);
	s.f.u = v;
	s.f.cur = g.voff[v];
	s.f.dist = distance + (int32_t)g.vlen[v];
	s.f.csat = csat;
	return SG_RUNNING;
}

// the whole search of one origin; SG_DONE, or the limit that stopped it
template <class Sat, class Stack, class Sink>
ABG_HD int sg_search(const SGGraph& g, uint32_t origin, const uint32_t* cv, const int32_t* cb, uint32_t nc, uint32_t max_cost, uint32_t max_paths,
    SGState<Sat>& s, Stack& st, Sink& sink)
{
	sg_begin(g, origin, s);
	int r;
	while ((r = sg_step(g, cv, cb, nc, max_cost, max_paths, s, st, sink)) == SG_RUNNING) { }
	return r;
}

} // namespace abg

// ---- host only from here
#include <algorithm>
#include <numeric>
#include <vector>

namespace abg {

struct SGHostSat {
	std::vector<uint8_t> m;
	bool test(uint32_t i) const { return m[i] != 0; }
	void set(uint32_t i) { m[i] = 1; }
	void clear(uint32_t i) { m[i] = 0; }
	void reset() { std::fill(m.begin(), m.end(), 0); }
};
struct SGHostStack {
	std::vector<SGFrame> v;
	uint32_t cap() const { return 0xFFFFFFFFu; }
	void store(uint32_t i, const SGFrame& f) { if (i >= v.size()) v.resize((size_t)i + 1); v[i] = f; }
	SGFrame load(uint32_t i) const { return v[i]; }
	uint32_t vertex(uint32_t i) const { return v[i].u; }
};
// paths appended to `nodes`, one end offset a path
struct SGHostSink {
	std::vector<uint32_t>* nodes;
	std::vector<uint64_t>* ends;
	bool emit(const SGHostStack& st, uint32_t depth, uint32_t top, uint32_t v)
	{
		for (uint32_t i = 1; i < depth; ++i) nodes->push_back(st.vertex(i));
		if (depth > 0) nodes->push_back(top);
		nodes->push_back(v);
		ends->push_back(nodes->size());
		return true;
	}
};

// sort(constraints) of ConstrainedSearch.h:134 on pair<ContigNode, int>: by vertex, then by bound
inline void sg_sort_constraints(uint32_t* cv, int32_t* cb, uint32_t nc)
{
	std::vector<uint32_t> order(nc);
	std::iota(order.begin(), order.end(), 0u);
	std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return cv[a] != cv[b] ? cv[a] < cv[b] : cb[a] < cb[b]; });
	std::vector<uint32_t> v(nc);
	std::vector<int32_t> b(nc);
	for (uint32_t i = 0; i < nc; ++i) { v[i] = cv[order[i]]; b[i] = cb[order[i]]; }
	std::copy(v.begin(), v.end(), cv);
	std::copy(b.begin(), b.end(), cb);
}

// one search on the host, with no limit but memory: its paths are appended to nodes / ends
inline void sg_search_host(const SGGraph& g, uint32_t origin, const uint32_t* cv, const int32_t* cb, uint32_t nc, uint32_t max_cost, uint32_t max_paths,
    uint32_t* visited, std::vector<uint32_t>& nodes, std::vector<uint64_t>& ends)
{
	SGState<SGHostSat> s;
	s.sat.m.assign(nc, 0);
	SGHostStack st;
	SGHostSink sink{ &nodes, &ends };
	(void)sg_search(g, origin, cv, cb, nc, max_cost, max_paths, s, st, sink);
	*visited = s.visited;
}

} // namespace abg
