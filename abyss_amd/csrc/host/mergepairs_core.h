// mergepairs_core.h -- abyss-mergepairs (Align/mergepairs.cc of the reference) around an aligner: options, the two readers, the
// batches, mergeReads, the three output files, stdout and the statistics.  abyss_amd/bin/abyss-mergepairs gives it the GPU
// (abg_mp_align), tests/hostcheck/mp_check the serial body of abg_mp.h.
//
// Kept from the reference on purpose:
//   - opt::trimMasked is 1 unless --no-trim-masked is given (DataLayer/FastaReader.cpp:29; the usage text says otherwise)
//   - --length1 and --length2 take no argument (longopts declares them no_argument): they set the length to 0
//   - each reader filters unchaste records on its own, so the pairing shifts where only one mate is filtered
//   - the output goes through std::ofstream and std::cout in the reference's order of operator<<
// Where the reference ends in an assert or an uncaught exception (a byte reverseComplement or isMatch refuses, files of unequal
// record count, -1 / -2 beyond a read's length) this prints the reference's lines, one line of its own, and exits 1.
#pragma once
#include "../abg_mp.h"
#include "fasta_reader.h"
#include "host_cli.h"

#include <getopt.h>

#include <fstream>
#include <iostream>
#include <sstream>

#ifndef ABG_IO_VERSION
#define ABG_IO_VERSION "2.3.10"
#endif
#define ABG_MP_PROGRAM "abyss-mergepairs"

namespace mp {

static const char VERSION_MESSAGE[] =
    ABG_MP_PROGRAM " (ABySS) " ABG_IO_VERSION "\n"
    "Written by Anthony Raymond.\n"
    "\n"
    "Copyright 2014 Canada's Michael Smith Genome Sciences Centre\n";

static const char USAGE_MESSAGE[] =
    "Usage: " ABG_MP_PROGRAM " [OPTION]... READS1 READS2\n"
    "Attempt to merge reads in READS1 with reads in READS2\n"
    "\n"
    " Options:\n"
    "\n"
    "  -o, --prefix=PREFIX     the prefix of all output files [out]\n"
    "  -p, --identity=N        minimum overlap identity [0.9]\n"
    "  -m, --matches=N         minimum number of matches in overlap [10]\n"
    "  -1, --length1=N         trim bases from 3' end of first read\n"
    "                          down to a maximum of N bp long [inf]\n"
    "  -2, --length2=N         trim bases from 3' end of second read\n"
    "                          down to a maximum of N bp long [inf]\n"
    "      --chastity          discard unchaste reads [default]\n"
    "      --no-chastity       do not discard unchaste reads\n"
    "      --trim-masked       trim masked bases from the ends of reads\n"
    "      --no-trim-masked    do not trim masked bases from the ends\n"
    "                          of reads [default]\n"
    "  -q, --trim-quality=N    trim bases from the ends of reads whose\n"
    "                          quality is less than the threshold\n"
    "      --standard-quality  zero quality is `!' (33)\n"
    "                          default for FASTQ and SAM files\n"
    "      --illumina-quality  zero quality is `@' (64)\n"
    "                          default for qseq and export files\n"
    "  -v, --verbose           display verbose output\n"
    "      --help              display this help and exit\n"
    "      --version           output version information and exit\n"
    "\n"
    "Report bugs to <abyss-users@bcgsc.ca>.\n";

struct Record { std::string id, comment, seq, qual; };

struct Options { // namespace opt, mergepairs.cc:59-69, and the reader's
	std::string prefix = "out";
	float identity = 0.9f;
	unsigned min_matches = 10;
	int max_len_1 = 0, max_len_2 = 0, verbose = 0;
	abghost::ReaderOptions reader;
	std::string reads1, reads2;
};

// What aligns a batch: read 1 of each of the first n pairs against the reverse complement of read 2 (r2 as the file holds it, rc2
// already complemented), one record a pair
struct Aligner {
	virtual ~Aligner() { }
	virtual bool open(std::string& err) = 0;
	virtual bool align(const std::vector<Record>& r1, const std::vector<Record>& r2, const std::vector<std::string>& rc2, size_t n, unsigned min_matches, float identity,
	    std::vector<abg::MPRecord>& out, std::string& err) = 0;
	virtual void close() { }
	// for the tests: order-dependent pairs, pairs whose loop took the early break, pairs whose loop did not
	uint64_t order_dependent = 0, break_taken = 0, break_not_taken = 0;
	void count(const abg::MPRecord& r)
	{
		order_dependent += (r.flags & abg::MP_ORDER_DEPENDENT) != 0;
		break_taken += (r.flags & abg::MP_BREAK_TAKEN) != 0;
		break_not_taken += (r.flags & abg::MP_BREAK_NOT_TAKEN) != 0;
	}
};

// main()'s option loop, mergepairs.cc:279-319.  false: the process ends with *status.
inline bool parse_options(int argc, char** argv, Options& o, int* status)
{
	static int chastityFilter, trimMasked, qualityOffset;
	chastityFilter = o.reader.chastityFilter;
	trimMasked = o.reader.trimMasked;
	qualityOffset = o.reader.qualityOffset;
	enum { OPT_HELP = 1, OPT_VERSION };
	static const struct option longopts[] = {
		{ "prefix", required_argument, NULL, 'o' },
		{ "identity", required_argument, NULL, 'p' },
		{ "matches", required_argument, NULL, 'm' },
		{ "verbose", no_argument, NULL, 'v' },
		{ "length1", no_argument, NULL, '1' },
		{ "length2", no_argument, NULL, '2' },
		{ "chastity", no_argument, &chastityFilter, 1 },
		{ "no-chastity", no_argument, &chastityFilter, 0 },
		{ "trim-masked", no_argument, &trimMasked, 1 },
		{ "no-trim-masked", no_argument, &trimMasked, 0 },
		{ "trim-quality", required_argument, NULL, 'q' },
		{ "standard-quality", no_argument, &qualityOffset, 33 },
		{ "illumina-quality", no_argument, &qualityOffset, 64 },
		{ "help", no_argument, NULL, OPT_HELP },
		{ "version", no_argument, NULL, OPT_VERSION },
		{ NULL, 0, NULL, 0 }
	};
	bool die = false;
	for (int c; (c = getopt_long(argc, argv, "o:p:m:q:1:2:v", longopts, NULL)) != -1;) {
		std::istringstream arg(optarg != NULL ? optarg : "");
		switch (c) {
		case '?': die = true; break;
		case 'o': arg >> o.prefix; break;
		case 'p': arg >> o.identity; break;
		case 'm': arg >> o.min_matches; break;
		case 'q': arg >> o.reader.qualityThreshold; break;
		case '1': arg >> o.max_len_1; break;
		case '2': arg >> o.max_len_2; break;
		case 'v': o.verbose++; break;
		case OPT_HELP: fputs(USAGE_MESSAGE, stdout); *status = EXIT_SUCCESS; return false;
		case OPT_VERSION: fputs(VERSION_MESSAGE, stdout); *status = EXIT_SUCCESS; return false;
		}
		if (optarg != NULL && !arg.eof()) {
			*status = cli::invalid_option(ABG_MP_PROGRAM, c, optarg);
			return false;
		}
	}
	o.reader.chastityFilter = chastityFilter;
	o.reader.trimMasked = trimMasked;
	o.reader.qualityOffset = qualityOffset;
	o.reader.foldCase = 0; // FastaReader::NO_FOLD_CASE
	if (argc - optind < 2) { fprintf(stderr, ABG_MP_PROGRAM ": missing arguments\n"); die = true; }
	if (argc - optind > 2) { fprintf(stderr, ABG_MP_PROGRAM ": too many arguments\n"); die = true; }
	if (die) {
		cli::try_help(ABG_MP_PROGRAM);
		*status = EXIT_FAILURE;
		return false;
	}
	o.reads1 = argv[optind++];
	o.reads2 = argv[optind++];
	return true;
}

// operator<<(ostream&, const FastqRecord&), DataLayer/FastaReader.h:156-196
inline void write_record(std::ostream& out, const Record& r)
{
	out << (r.qual.empty() ? '>' : '@') << r.id;
	if (!r.comment.empty()) out << ' ' << r.comment;
	if (r.qual.empty()) out << '\n' << r.seq << '\n';
	else out << '\n' << r.seq << "\n" "+\n" << r.qual << '\n';
}

// mergeReads, mergepairs.cc:113-160, from the overlap's t_pos, h_pos and length alone
inline void merge_reads(const abg::MPRecord& o, const Record& rec1, const std::string& rc_seq2, const Record& rec2, Record& out)
{
	const size_t ol = o.length;
	const std::string& seq1 = rec1.seq;
	const std::string& qual1 = rec1.qual;
	const std::string rc_qual2(rec2.qual.rbegin(), rec2.qual.rend());
	const size_t out_len = o.t_pos + ol + rc_seq2.length() - o.h_pos - 1;
	std::string out_seq(out_len, 'N'), out_qual(out_len, '#');
	std::copy(seq1.begin(), seq1.begin() + o.t_pos, out_seq.begin());
	std::copy(rc_seq2.begin() + o.h_pos + 1, rc_seq2.end(), out_seq.begin() + o.t_pos + ol);
	if (qual1.size() == seq1.size() && rc_qual2.size() == rc_seq2.size()) {
		std::copy(qual1.begin(), qual1.begin() + o.t_pos, out_qual.begin());
		std::copy(rc_qual2.begin() + ol, rc_qual2.end(), out_qual.begin() + seq1.length());
	}
	for (unsigned i = 0; i < ol; i++) {
		const unsigned pos = (unsigned)(seq1.length() - ol + i);
		const bool q = qual1.size() == seq1.size() && rc_qual2.size() == rc_seq2.size();
		const char qa = q ? qual1[pos] : '#', qb = q ? rc_qual2[i] : '#';
		if (seq1[pos] == rc_seq2[i]) {
			out_seq[pos] = seq1[pos];
			out_qual[pos] = std::max(qa, qb);
		} else {
			out_seq[pos] = qa > qb ? seq1[pos] : rc_seq2[i]; // bestBase
			out_qual[pos] = std::min(qa, qb);
		}
	}
	out.id = rec1.id;
	out.comment = rec1.comment;
	out.seq = out_seq;
	out.qual = out_qual;
}

// printAlignment of the first alignment the loop finds (smith_waterman.cpp:33-52, 96-168), for -vvv: the whole matrix of moves
inline void print_first_alignment(const std::string& a, const std::string& b, unsigned min_matches, const uint32_t* min_identity, abg::MPRecord& r, std::string& log)
{
	std::vector<abg::MPCell> row;
	std::vector<uint8_t> which;
	abg::mp_last_row_host(a, b, row, &which);
	abg::MPRecord probe;
	abg::mp_select(row.data(), (uint32_t)a.size(), (uint32_t)b.size(), min_matches, min_identity, probe, abg::MPSerial());
	const uint32_t jmax = abg::mp_replay(row.data(), (uint32_t)a.size(), (uint32_t)b.size(), min_matches, min_identity, r);
	r.flags |= probe.flags & abg::MP_ORDER_DEPENDENT;
	if (!jmax) return;
	const size_t lb = b.size();
	std::string qa, ta, match;
	auto pair = [&](size_t i, size_t j) {
		char c;
		if (abg::mc_detail::is_match(a[i - 1], b[j - 1], c)) match += c;
		else match += abg::mc_detail::ambiguity(a[i - 1], b[j - 1], true);
	};
	size_t ci = a.size(), cj = jmax;
	for (;;) {
		const uint8_t w = which[(ci - 1) * lb + (cj - 1)];
		const size_t ni = w == 2 ? ci : ci - 1, nj = w == 1 ? cj : cj - 1;
		if (ni == 0 || nj == 0) break;
		if (w == 2) { qa += '-'; match += (char)tolower((unsigned char)b[cj - 1]); ta += b[cj - 1]; }
		else {
			qa += a[ci - 1];
			if (w == 1) { ta += '-'; match += (char)tolower((unsigned char)a[ci - 1]); }
			else { ta += b[cj - 1]; pair(ci, cj); }
		}
		ci = ni;
		cj = nj;
	}
	qa += a[ci - 1];
	ta += b[cj - 1];
	pair(ci, cj);
	std::reverse(qa.begin(), qa.end());
	std::reverse(ta.begin(), ta.end());
	std::reverse(match.begin(), match.end());
	const size_t astart = ci - 1;
	log += a.substr(0, astart) + qa + '\n' + std::string(astart, ' ');
	for (size_t i = 0; i < match.size(); i++) log += (match[i] == qa[i] || match[i] == ta[i]) ? '.' : match[i];
	log += '\n' + std::string(astart, ' ') + ta + b.substr(jmax) + '\n';
}

[[noreturn]] inline void reference_aborts(Aligner& al, const char* what)
{
	al.close();
	std::cout.flush();
	fprintf(stderr, ABG_MP_PROGRAM ": error: %s\n", what);
	exit(EXIT_FAILURE);
}

// pairs read before they are aligned: four of the aligner's batches (ABG_MP_BATCH, include/abyss_amd.h), so that its two streams
// have batches to alternate between
inline uint64_t batch_size()
{
	const char* v = getenv("ABG_MP_BATCH");
	const unsigned long long n = v && *v ? strtoull(v, nullptr, 10) : 0;
	return 4 * (n ? std::min<unsigned long long>(n, 1ull << 22) : (1ull << 16));
}

inline int run_main(int argc, char** argv, Aligner& al)
{
	Options o;
	int status = 0;
	if (!parse_options(argc, argv, o, &status)) return status;

	// alignFiles, mergepairs.cc:208-267
	if (o.verbose > 0) std::cerr << "Merging `" << o.reads1 << "' with `" << o.reads2 << "'\n";
	abghost::FastaReader r1(o.reads1, o.reader);
	r1.set_max_length(o.max_len_1);
	abghost::FastaReader r2(o.reads2, o.reader);
	r2.set_max_length(o.max_len_2);
	std::ofstream unmerged1((o.prefix + "_reads_1.fastq").c_str());
	std::ofstream unmerged2((o.prefix + "_reads_2.fastq").c_str());
	std::ofstream merged((o.prefix + "_merged.fastq").c_str());

	struct { unsigned total_reads = 0, merged_reads = 0, unmerged_reads = 0, unchaste_reads = 0, no_alignment = 0, too_many_aligns = 0, low_matches = 0, has_indel = 0, pid_low = 0; } stats;
	const uint64_t batch = batch_size();
	std::vector<Record> b1, b2;
	std::vector<std::string> rc2;
	std::vector<abg::MPRecord> recs;
	std::vector<uint32_t> min_identity;
	std::string err;
	bool opened = false, more = true;
	const char* ends = nullptr; // why the reference would end here, once the pairs before it are written
	std::string ends_line;      // and what it prints itself as it does
	int x = 0;
	while (more) {
		// a batch of pairs, up to the record at which the reference would have ended
		size_t n = 0;
		for (; n < batch; n++) {
			if (b1.size() <= n) { b1.emplace_back(); b2.emplace_back(); rc2.emplace_back(); }
			Record &p = b1[n], &q = b2[n];
			const bool got1 = r1.read(p.id, p.comment, p.seq, p.qual);
			if (got1 && r1.beyond()) { ends = "-1 is beyond a read's length, which the reference does not survive (basic_string::erase)"; more = false; break; }
			const bool got2 = got1 && r2.read(q.id, q.comment, q.seq, q.qual);
			if (got2 && r2.beyond()) { ends = "-2 is beyond a read's length, which the reference does not survive (basic_string::erase)"; more = false; break; }
			if (!got2) {
				// `r2 >> rec2` once more, then assert(r1.eof()), assert(r2.eof()): neither holds after a record has been read
				Record extra;
				if (got1 || r2.read(extra.id, extra.comment, extra.seq, extra.qual)) ends = "the two files hold different numbers of records, where the reference asserts";
				more = false;
				break;
			}
			bool bad = false;
			for (char c : q.seq)
				if (!abg::ov_complement((uint8_t)c)) { // complementBaseChar, Common/Sequence.cpp:41-44
					ends_line = std::string("error: unexpected character: `") + c + "'\n";
					ends = "a read holds a character that has no complement, where the reference asserts";
					bad = true;
					break;
				}
			if (bad) { more = false; break; }
			rc2[n] = abg::mp_reverse_complement(q.seq);
			if (abg::mp_pair_asserts(p.seq, rc2[n])) { ends = "a read holds a character that is no nucleotide code, where the reference asserts"; more = false; break; }
			if (std::max(p.seq.size(), q.seq.size()) > abg::MP_MAX_READ) { ends = "a read is longer than 100,000 bases"; more = false; break; }
		}
		if (n > 0) {
			uint32_t longest = 0;
			for (size_t i = 0; i < n; i++) longest = std::max<uint32_t>(longest, (uint32_t)(b1[i].seq.size() + rc2[i].size()));
			if (min_identity.size() < (size_t)longest + 1) min_identity = abg::mp_identity_table(o.identity, longest);
			recs.assign(n, abg::MPRecord{ 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 });
			if (o.verbose <= 2) {
				if (!opened && !al.open(err)) { fprintf(stderr, ABG_MP_PROGRAM ": error: %s\n", err.c_str()); return EXIT_FAILURE; }
				opened = true;
				if (!al.align(b1, b2, rc2, n, o.min_matches, o.identity, recs, err)) { fprintf(stderr, ABG_MP_PROGRAM ": error: %s\n", err.c_str()); return EXIT_FAILURE; }
			}
		}
		for (size_t i = 0; i < n; i++) {
			stats.total_reads++;
			abg::MPRecord& r = recs[i];
			if (o.verbose > 2) { // the alignment's print needs the whole matrix: the host's, pair by pair
				std::string log;
				print_first_alignment(b1[i].seq, rc2[i], o.min_matches, min_identity.data(), r, log);
				std::cerr << log;
			}
			al.count(r);
			// filterAlignments, mergepairs.cc:167-205: the statistic of the stage that empties the list
			if (r.n_aligned == 0) stats.no_alignment++;
			else if (r.n_matches == 0) stats.low_matches++;
			else if (r.n_identity == 0) stats.pid_low++;
			else if (r.n_gapless == 0) stats.has_indel++;
			if (r.n_gapless == 1) {
				stats.merged_reads++;
				Record out;
				merge_reads(r, b1[i], rc2[i], b2[i], out);
				write_record(merged, out);
				std::cout << r.length << ' ' << r.matches << '\n';
			} else {
				if (r.n_gapless > 1) stats.too_many_aligns++;
				stats.unmerged_reads++;
				write_record(unmerged1, b1[i]);
				write_record(unmerged2, b2[i]);
			}
			if (o.verbose > 0 && ++x % 10000 == 0) std::cerr << "Aligned " << x << " reads.\n";
		}
	}
	if (ends) {
		std::cerr << ends_line;
		reference_aborts(al, ends);
	}
	stats.unchaste_reads = r1.unchaste();
	stats.total_reads += r1.unchaste();
	unmerged1.close();
	unmerged2.close();
	merged.close();
	al.close();

	std::cerr << "Pair merging stats: total=" << stats.total_reads << " merged=" << stats.merged_reads << " unmerged=" << stats.unmerged_reads
	          << " unchaste=" << stats.unchaste_reads << '\n'
	          << "no_alignment=" << stats.no_alignment << " too_many_aligns=" << stats.too_many_aligns << " too_few_matches=" << stats.low_matches
	          << " has_indel=" << stats.has_indel << " low_pid=" << stats.pid_low << '\n';
	return 0;
}

} // namespace mp
