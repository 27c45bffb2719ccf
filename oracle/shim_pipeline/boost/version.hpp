// Stand-in for <boost/version.hpp>: the subset the reference's abyss-map, abyss-index, abyss-fixmate, DistanceEst and Overlap use
// (the same text tests/golden/make_{map,distanceest,overlap}.py write).  TEST INFRASTRUCTURE ONLY.
#pragma once
#define BOOST_VERSION 106000
