// Stand-in for <boost/lambda/lambda.hpp>: the subset the reference's abyss-map, abyss-index, abyss-fixmate, DistanceEst and Overlap use
// (the same text tests/golden/make_{map,distanceest,overlap}.py write).  TEST INFRASTRUCTURE ONLY.
#pragma once
namespace boost { namespace lambda {
struct placeholder1_ { };
static const placeholder1_ _1 = placeholder1_();
template <class F, class A, class B> struct bound_ {
	F f; A a; B b;
	template <class E> bool operator()(const E& e) const { return f(a.get(), b.get(), e); }
};
template <class T> struct not_ { T t; template <class E> bool operator()(const E& e) const { return !t(e); } };
template <class F, class A, class B> not_<bound_<F, A, B> > operator!(const bound_<F, A, B>& b) { not_<bound_<F, A, B> > n = { b }; return n; }
template <class F, class A, class B> bound_<F, A, B> bind(F f, A a, B b, placeholder1_) { bound_<F, A, B> x = { f, a, b }; return x; }
} }
