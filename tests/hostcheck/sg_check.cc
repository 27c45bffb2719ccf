// sg_check -- SimpleGraph without a GPU, for the CPU suite: the same simplegraph_core.h as abyss_amd/bin/SimpleGraph over the search
// body of abg_sg.h run serially (what the kernel must equal).
//   sg_check run ARGS...        what `SimpleGraph ARGS...` writes (stdout, the -o file, stderr, status)
//   sg_check search IN OUT      the search for a search file
// A search file, little-endian: u64 nv, u64 eoff[nv + 1], u32 len[nv], u32 target[ne], i32 distance[ne], u32 max_cost, u32 max_paths,
// u64 nsearch, u32 origin[nsearch], u64 coff[nsearch + 1], u32 cvertex[nc], i32 cbound[nc].  The result file: per search u32 visited,
// u32 npaths, then per path u32 length and its vertices.
#include "../../abyss_amd/csrc/abg_sg.h"
#include "../../abyss_amd/csrc/host/simplegraph_core.h"

namespace {

struct SerialSearcher : sg::Searcher {
	std::vector<uint32_t> voff, vlen, etgt;
	std::vector<int32_t> edist;
	bool open(std::string&) override { return true; }
	bool set_graph(const std::vector<uint64_t>& eoff, const std::vector<uint32_t>& lengths, const std::vector<uint32_t>& targets,
	    const std::vector<int32_t>& distances, std::string&) override
	{
		voff.assign(eoff.begin(), eoff.end());
		vlen = lengths;
		etgt = targets;
		edist = distances;
		return true;
	}
	bool search(const std::vector<uint32_t>& origins, const std::vector<uint64_t>& coff, const std::vector<uint32_t>& cv0, const std::vector<int32_t>& cb0,
	    uint32_t max_cost, uint32_t max_paths, std::vector<uint32_t>& visited, std::vector<uint64_t>& index, std::vector<uint64_t>& poff,
	    std::vector<uint32_t>& nodes, std::string& err) override
	{
		const abg::SGGraph g{ voff.data(), vlen.data(), etgt.data(), edist.data(), (uint32_t)vlen.size() };
		std::vector<uint32_t> cv(cv0);
		std::vector<int32_t> cb(cb0);
		visited.assign(origins.size(), 0);
		index.assign(1, 0);
		poff.assign(1, 0);
		nodes.clear();
		std::vector<uint64_t> ends;
		for (size_t i = 0; i < origins.size(); ++i) {
			if (origins[i] >= g.nv) { err = "search " + std::to_string(i) + ": no such vertex"; return false; }
			const uint32_t nc = (uint32_t)(coff[i + 1] - coff[i]);
			if (nc > 0) { // (ConstrainedSearch.h:130-131: no constraint, no search)
				abg::sg_sort_constraints(cv.data() + coff[i], cb.data() + coff[i], nc);
				ends.clear();
				abg::sg_search_host(g, origins[i], cv.data() + coff[i], cb.data() + coff[i], nc, max_cost, max_paths, &visited[i], nodes, ends);
				poff.insert(poff.end(), ends.begin(), ends.end());
			}
			index.push_back(poff.size() - 1);
		}
		return true;
	}
};

template <class T> bool get(FILE* f, std::vector<T>& v, size_t n) { v.resize(n); return n == 0 || fread(v.data(), sizeof(T), n, f) == n; }

int search(const char* in, const char* out)
{
	FILE* f = fopen(in, "rb");
	if (!f) { fprintf(stderr, "sg_check: cannot read %s\n", in); return 2; }
	uint64_t nv = 0, ns = 0;
	uint32_t cost = 0, paths = 0;
	std::vector<uint64_t> eoff, coff;
	std::vector<uint32_t> len, tgt, origins, cv;
	std::vector<int32_t> dist, cb;
	bool ok = fread(&nv, 8, 1, f) == 1 && get(f, eoff, nv + 1) && get(f, len, nv) && get(f, tgt, eoff[nv]) && get(f, dist, eoff[nv]);
	ok = ok && fread(&cost, 4, 1, f) == 1 && fread(&paths, 4, 1, f) == 1 && fread(&ns, 8, 1, f) == 1 && get(f, origins, ns) && get(f, coff, ns + 1);
	ok = ok && get(f, cv, coff[ns]) && get(f, cb, coff[ns]);
	fclose(f);
	if (!ok) { fprintf(stderr, "sg_check: %s is cut short\n", in); return 2; }
	SerialSearcher s;
	std::string err;
	std::vector<uint32_t> visited, nodes;
	std::vector<uint64_t> index, poff;
	if (!s.set_graph(eoff, len, tgt, dist, err) || !s.search(origins, coff, cv, cb, cost, paths, visited, index, poff, nodes, err)) {
		fprintf(stderr, "sg_check: %s\n", err.c_str());
		return 2;
	}
	FILE* o = fopen(out, "wb");
	if (!o) { fprintf(stderr, "sg_check: cannot write %s\n", out); return 2; }
	for (size_t i = 0; i < origins.size(); ++i) {
		const uint32_t np = (uint32_t)(index[i + 1] - index[i]);
		fwrite(&visited[i], 4, 1, o);
		fwrite(&np, 4, 1, o);
		for (uint64_t p = index[i]; p < index[i + 1]; ++p) {
			const uint32_t l = (uint32_t)(poff[p + 1] - poff[p]);
			fwrite(&l, 4, 1, o);
			fwrite(&nodes[poff[p]], 4, l, o);
		}
	}
	return fclose(o) == 0 ? 0 : 2;
}

} // namespace

int main(int argc, char** argv)
{
	const std::string mode = argc > 1 ? argv[1] : "";
	if (mode == "run") {
		SerialSearcher s;
		argv[1] = argv[0];
		return sg::run_main(argc - 1, argv + 1, s);
	}
	if (mode == "search" && argc == 4) return search(argv[2], argv[3]);
	fprintf(stderr, "usage: sg_check run ARGS... | search IN OUT\n");
	return 2;
}
