// Stand-in for the part of glm's public interface (glm 0.9.6, the version the reference vendors) that the reference's call
// sites in tests/shim_callsites.cpp use: glm::vec3 / glm::mat3 as the templates tvec3 / tmat3x3 with a precision
// parameter, column-major storage (m[col][row]), a default mat3 that is the identity, element access, comparison and the
// basic arithmetic.  Written for the compile-only shim test when no glm is installed; a real glm is used when one is found
// (tests/test_host_boundary.py).  It defines GLM_VERSION like glm does, so include/goicp_mi355.hpp takes its glm branch.
#ifndef GOICP_TESTS_GLM_API_GLM_HPP
#define GOICP_TESTS_GLM_API_GLM_HPP

#define GLM_VERSION 96

#include <cstddef>

namespace glm {

enum precision { highp, mediump, lowp, defaultp = highp };
typedef int length_t;

template <typename T, precision P = defaultp>
struct tvec3 {
	typedef T value_type;
	T x, y, z;
	tvec3() : x(0), y(0), z(0) {}
	explicit tvec3(T s) : x(s), y(s), z(s) {}
	tvec3(T a, T b, T c) : x(a), y(b), z(c) {}
	static length_t length() { return 3; }
	T& operator[](length_t i) { return (&x)[i]; }
	const T& operator[](length_t i) const { return (&x)[i]; }
	tvec3& operator+=(const tvec3& v) { x += v.x; y += v.y; z += v.z; return *this; }
	tvec3& operator-=(const tvec3& v) { x -= v.x; y -= v.y; z -= v.z; return *this; }
	tvec3& operator*=(T s) { x *= s; y *= s; z *= s; return *this; }
};
template <typename T, precision P> bool operator==(const tvec3<T, P>& a, const tvec3<T, P>& b) { return a.x == b.x && a.y == b.y && a.z == b.z; }
template <typename T, precision P> bool operator!=(const tvec3<T, P>& a, const tvec3<T, P>& b) { return !(a == b); }
template <typename T, precision P> tvec3<T, P> operator+(tvec3<T, P> a, const tvec3<T, P>& b) { return a += b; }
template <typename T, precision P> tvec3<T, P> operator-(tvec3<T, P> a, const tvec3<T, P>& b) { return a -= b; }
template <typename T, precision P> tvec3<T, P> operator*(tvec3<T, P> a, T s) { return a *= s; }
template <typename T, precision P> tvec3<T, P> operator*(T s, tvec3<T, P> a) { return a *= s; }

template <typename T, precision P = defaultp>
struct tmat3x3 {
	typedef tvec3<T, P> col_type;
	typedef tvec3<T, P> row_type;
	typedef T value_type;
	col_type value[3];
	tmat3x3() : tmat3x3(T(1)) {}
	explicit tmat3x3(T s) { value[0] = col_type(s, 0, 0); value[1] = col_type(0, s, 0); value[2] = col_type(0, 0, s); }
	tmat3x3(const col_type& c0, const col_type& c1, const col_type& c2) { value[0] = c0; value[1] = c1; value[2] = c2; }
	static length_t length() { return 3; }
	col_type& operator[](length_t i) { return value[i]; }
	const col_type& operator[](length_t i) const { return value[i]; }
};
template <typename T, precision P> bool operator==(const tmat3x3<T, P>& a, const tmat3x3<T, P>& b) { return a[0] == b[0] && a[1] == b[1] && a[2] == b[2]; }
template <typename T, precision P> bool operator!=(const tmat3x3<T, P>& a, const tmat3x3<T, P>& b) { return !(a == b); }
template <typename T, precision P> tvec3<T, P> operator*(const tmat3x3<T, P>& m, const tvec3<T, P>& v) { return m[0] * v.x + m[1] * v.y + m[2] * v.z; }
template <typename T, precision P> tmat3x3<T, P> operator*(const tmat3x3<T, P>& a, const tmat3x3<T, P>& b) { return tmat3x3<T, P>(a * b[0], a * b[1], a * b[2]); }

typedef tvec3<float, highp> highp_vec3;
typedef tmat3x3<float, highp> highp_mat3;
typedef highp_vec3 vec3;
typedef highp_mat3 mat3;
typedef highp_mat3 mat3x3;

}  // namespace glm

#endif
