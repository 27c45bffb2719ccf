// host_cli.h -- the frame the drop-in binaries' option loops and error exits share: the command line as the SAM header quotes it, the
// two lines every ABySS program ends a bad command line with, and the error exit of the cores.  The option tables and switches are
// each program's own: they restate the reference's main line by line.
#pragma once

#include <cstdio>
#include <cstdlib>
#include <string>

namespace cli {

// the arguments joined by one space (opt::commandLine of the reference's mains)
inline std::string command_line(int argc, char** argv)
{
	std::string s;
	for (int i = 0; i < argc; i++) { if (i) s += ' '; s += argv[i]; }
	return s;
}

// an option's argument that did not parse to its end; the status to leave with
inline int invalid_option(const char* program, int c, const char* optarg)
{
	fprintf(stderr, "%s: invalid option: `-%c%s'\n", program, (char)c, optarg);
	return EXIT_FAILURE;
}

inline void try_help(const char* program) { fprintf(stderr, "Try `%s --help' for more information.\n", program); }

// where the reference aborts or trips an assert: stdout first, so that the two streams keep their order in a shared file
[[noreturn]] inline void fail(const char* program, const std::string& msg)
{
	fflush(stdout);
	fprintf(stderr, "%s: error: %s\n", program, msg.c_str());
	exit(EXIT_FAILURE);
}

} // namespace cli
