// bloom_core.h -- the host side of Konnector Bloom filter files (`abyss-bloom build -t konnector`, union, intersect, info,
// compare, kmers): the file header, the bit-level reads that place a file's window into a filter, popcount and the statistics
// lines.  Plain C++: union / intersect / info / compare never start the HIP runtime.
//
// Reference behaviour restated here:
//   Bloom/Bloom.h writeHeader / readHeader   "5\n<k>\n<fullBits>\t<start>\t<end>\n<seed>\n", then ceil((end - start + 1) / 8) bytes
//   Common/BitUtil.h readBits / copyBits     a file's bits placed at bit `start` of the filter, overwritten, ORed or ANDed in
//   Bloom/BloomFilter.h popcount             whole 64-bit words of the byte array, then bit by bit up to the size
//   Bloom/bloom.cc printBloomStats /
//                  printCascadingBloomStats  the statistics lines (FPR = popcount / size, 3 significant digits)
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

namespace kn {

constexpr unsigned BLOOM_VERSION = 5;

struct Header {
	unsigned version = 0, k = 0;
	uint64_t full = 0, start = 0, end = 0, seed = 0;
	uint64_t bits() const { return end - start + 1; }
	uint64_t bytes() const { return (bits() + 7) / 8; }
};

inline void write_header(FILE* f, unsigned k, uint64_t full, uint64_t start, uint64_t end, uint64_t seed)
{
	fprintf(f, "%u\n%u\n%llu\t%llu\t%llu\n%llu\n", BLOOM_VERSION, k, (unsigned long long)full, (unsigned long long)start,
	    (unsigned long long)end, (unsigned long long)seed);
}

[[noreturn]] inline void die(const std::string& msg)
{
	fputs(msg.c_str(), stderr);
	fflush(stdout);
	exit(EXIT_FAILURE);
}

// Bloom::readHeader: the reference's messages (and status 1) for a version or k that does not match; a header that does not
// parse ends the run with a message too (the reference stops at an assertion there)
inline Header read_header(FILE* f, const std::string& path, unsigned k)
{
	Header h;
	unsigned long long full = 0, start = 0, end = 0, seed = 0;
	if (fscanf(f, "%u", &h.version) != 1 || fgetc(f) != '\n') die("error: `" + path + "': not a Bloom filter file\n");
	if (h.version != BLOOM_VERSION)
		die("error: bloom filter version (`" + std::to_string(h.version) + "'), does not match version required by this program (`5').\n");
	if (fscanf(f, "%u", &h.k) != 1 || fgetc(f) != '\n') die("error: `" + path + "': not a Bloom filter file\n");
	if (h.k != k)
		die("error: this program must be run with the same kmer size as the bloom filter being loaded (k=" + std::to_string(h.k) + ").\n");
	if (fscanf(f, "%llu", &full) != 1 || fgetc(f) != '\t' || fscanf(f, "%llu", &start) != 1 || fgetc(f) != '\t' ||
	    fscanf(f, "%llu", &end) != 1 || fgetc(f) != '\n' || fscanf(f, "%llu", &seed) != 1 || fgetc(f) != '\n')
		die("error: `" + path + "': not a Bloom filter file\n");
	if (!(start < full && end < full && start <= end)) die("error: `" + path + "': bad Bloom filter dimensions\n");
	h.full = full; h.start = start; h.end = end; h.seed = seed;
	return h;
}

enum Op { OVERWRITE, OR, AND };

// readBits(in, dest, bits, offset, op) as the reference computes it, src holding the file's ceil(bits / 8) bytes.  dest needs one
// byte beyond the filter (the reference writes the byte after a window's last full byte).  With a window that does not start on a
// byte boundary the reference shifts a (signed) char right: a source byte whose top bit is set also sets the `offset % 8` top
// bits of its destination byte when overwriting or ORing.  That is kept, so that such files come out as the reference's do.
inline void read_bits(const uint8_t* src, uint8_t* dest, uint64_t bits, uint64_t offset, Op op)
{
	const uint64_t o = offset / 8, bytes = (bits + 7) / 8, fullb = bits % 8 ? bytes - 1 : bytes;
	const unsigned s = (unsigned)(offset % 8);
	const uint8_t carry = (uint8_t)(0xFFu << (8 - s)); // the top s bits of a destination byte: not this source byte's
	for (uint64_t i = 0; i < fullb; i++) {
		const uint8_t hi = (uint8_t)((int8_t)src[i] >> s), lo = (uint8_t)(src[i] << (8 - s));
		uint8_t& d0 = dest[o + i];
		uint8_t& d1 = dest[o + i + 1];
		if (op == AND) { d0 &= hi | carry; d1 &= lo | (uint8_t)~carry; continue; }
		if (op == OVERWRITE) { d0 &= carry; d1 &= (uint8_t)~carry; }
		d0 |= hi;
		d1 |= lo;
	}
	if (fullb < bytes) {
		const unsigned r = (unsigned)(bits % 8);
		const uint8_t mask = (uint8_t)(0xFFu << (8 - r)), lcarry = (uint8_t)(mask << (8 - s));
		const uint8_t last = src[bytes - 1] & mask;
		uint8_t& d0 = dest[o + bytes - 1];
		const uint8_t hi = (uint8_t)((int8_t)last >> s);
		if (op == OVERWRITE) d0 &= (uint8_t)~(mask >> s);
		if (op == AND) d0 &= hi | (uint8_t)~(mask >> s);
		else d0 |= hi;
		if (lcarry) {
			uint8_t& d1 = dest[o + bytes];
			const uint8_t lo = (uint8_t)(last << (8 - s));
			if (op == OVERWRITE) d1 &= (uint8_t)~lcarry;
			if (op == AND) d1 &= lo | (uint8_t)~lcarry;
			else d1 |= lo;
		}
	}
}

// reads a file's bits (after its header) and places them as read_bits does
inline void load_bits(FILE* f, const std::string& path, const Header& h, uint8_t* dest, uint64_t offset, Op op)
{
	std::vector<uint8_t> src(h.bytes());
	if (fread(src.data(), 1, src.size(), f) != src.size()) die("error: `" + path + "': the Bloom filter file is truncated\n");
	read_bits(src.data(), dest, h.bits(), offset, op);
}

inline uint64_t popcount(const uint8_t* a, uint64_t size)
{
	const uint64_t bytes = (size + 7) / 8, words = bytes / 8;
	uint64_t n = 0;
	for (uint64_t i = 0; i < words * 8; i++) n += (uint64_t)__builtin_popcount(a[i]);
	for (uint64_t i = words * 64; i < size; i++) n += (a[i / 8] >> (7 - i % 8)) & 1;
	return n;
}

inline std::string fpr(uint64_t pop, uint64_t size)
{
	char b[64];
	snprintf(b, sizeof b, "%.3g", 100 * ((double)pop / (double)size));
	return b;
}

inline std::string bloom_stats(uint64_t size, uint64_t pop)
{
	return "Bloom size (bits): " + std::to_string(size) + "\nBloom popcount (bits): " + std::to_string(pop) +
	       "\nBloom filter FPR: " + fpr(pop, size) + "%\n";
}

inline std::string cascading_stats(uint64_t size, const std::vector<uint64_t>& pops)
{
	std::string s;
	for (size_t i = 0; i < pops.size(); i++)
		s += "Stats for Bloom filter level " + std::to_string(i + 1) + ":\n\tBloom size (bits): " + std::to_string(size) +
		     "\n\tBloom popcount (bits): " + std::to_string(pops[i]) + "\n\tBloom filter FPR: " + fpr(pops[i], size) + "%\n";
	return s;
}

enum Format { FASTA, BED, RAW };

// bloom.cc memberOf: one printed k-mer (its characters are the read's, already upper case)
inline void format_kmer(std::string& out, Format fmt, const std::string& id, uint64_t seq_index, uint64_t i, unsigned k, const char* kmer)
{
	if (fmt == FASTA) {
		out += '>'; out += id; out += ":seq:"; out += std::to_string(seq_index); out += ":kmer:"; out += std::to_string(i); out += '\n';
	} else if (fmt == BED) {
		out += id; out += '\t'; out += std::to_string(i); out += '\t'; out += std::to_string(i + k - 1); out += '\t';
	}
	out.append(kmer, k);
	out += '\n';
}

} // namespace kn
