// Stand-in for <boost/integer.hpp>: the subset the reference's abyss-map, abyss-index, abyss-fixmate, DistanceEst and Overlap use
// (the same text tests/golden/make_{map,distanceest,overlap}.py write).  TEST INFRASTRUCTURE ONLY.
#pragma once
#include <stdint.h>
namespace boost {
template <int Bits> struct uint_t;
template <> struct uint_t<32> { typedef uint32_t least; };
template <> struct uint_t<64> { typedef uint64_t least; };
template <int Bits> struct int_t;
template <> struct int_t<32> { typedef int32_t least; };
template <> struct int_t<64> { typedef int64_t least; };
}
