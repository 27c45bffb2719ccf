// Stand-in for <boost/lambda/bind.hpp>: the subset the reference's abyss-map, abyss-index, abyss-fixmate, DistanceEst and Overlap use
// (the same text tests/golden/make_{map,distanceest,overlap}.py write).  TEST INFRASTRUCTURE ONLY.
#pragma once
#include <boost/lambda/lambda.hpp>
