// Stand-in for <boost/algorithm/string/join.hpp>: the subset the reference's abyss-map, abyss-index, abyss-fixmate, DistanceEst and Overlap use
// (the same text tests/golden/make_{map,distanceest,overlap}.py write).  TEST INFRASTRUCTURE ONLY.
#pragma once
#include <string>
namespace boost { namespace algorithm {
template <class Seq> std::string join(const Seq& v, const std::string& sep)
{
	std::string s;
	for (typename Seq::const_iterator it = v.begin(); it != v.end(); ++it) { if (it != v.begin()) s += sep; s += *it; }
	return s;
}
} }
