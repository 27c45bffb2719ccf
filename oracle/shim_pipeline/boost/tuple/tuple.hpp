// Stand-in for <boost/tuple/tuple.hpp>: the subset the reference's abyss-map, abyss-index, abyss-fixmate, DistanceEst and Overlap use
// (the same text tests/golden/make_{map,distanceest,overlap}.py write).  TEST INFRASTRUCTURE ONLY.
#pragma once
#include <tuple>
namespace boost {
using std::tie;
template <class A, class B> struct tuple;
template <int N, class A, class B> struct tuple_get_;
template <class A, class B> struct tuple_get_<0, A, B> { static A get(const tuple<A, B>& t) { return t.a; } };
template <class A, class B> struct tuple_get_<1, A, B> { static B get(const tuple<A, B>& t) { return t.b; } };
template <class A, class B> struct tuple {
	A a; B b;
	tuple(A a, B b) : a(a), b(b) { }
	template <int N> auto get() const -> decltype(tuple_get_<N, A, B>::get(*this)) { return tuple_get_<N, A, B>::get(*this); }
};
}
