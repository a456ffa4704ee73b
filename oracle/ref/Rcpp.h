/*
 * Rcpp.h -- this project's stand-in for the part of Rcpp's public interface that the reference's headers name.
 *
 * TEST INFRASTRUCTURE ONLY.  `make -C oracle ref` puts this directory in front of the reference's src/ so that its
 * FM.h compiles unmodified into oracle/_ref/ref_harness (see ref_harness.cpp).  Written from Rcpp's documented
 * interface (Rcpp-quickref, the Rcpp::List / Rcpp::Named / NumericVector reference pages), not from the reference and
 * not from Rcpp's sources: every type here is a plain std:: container with R's reference semantics (copies share
 * storage) and nothing talks to R.  What the harness does not reach is kept to the minimum that compiles.
 *
 * The two random entry points of R's C API, Rf_rnorm and Rf_rgamma, are only DECLARED here: ref_harness.cpp defines
 * them, deterministic and logged.
 */
#ifndef FMX_REF_RCPP_STANDIN_H_
#define FMX_REF_RCPP_STANDIN_H_

#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <limits>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

typedef struct SEXPREC* SEXP;

static const double R_PosInf = std::numeric_limits<double>::infinity();
static const double R_NegInf = -std::numeric_limits<double>::infinity();
static const double NA_REAL = std::numeric_limits<double>::quiet_NaN();
inline int R_IsNaN(double x) { return x != x; }
inline void Rf_warning(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  std::fprintf(stderr, "warning: ");
  std::vfprintf(stderr, fmt, ap);
  std::fprintf(stderr, "\n");
  va_end(ap);
}
double Rf_rnorm(double mean, double sd);
double Rf_rgamma(double shape, double scale);

namespace Rcpp {

inline void stop(const std::string& what) { throw std::runtime_error(what); }

/* a vector with R's sharing: a copy refers to the same storage */
template <typename T>
class SharedVector {
 public:
  typedef T* iterator;
  typedef const T* const_iterator;
  SharedVector() : d_(std::make_shared<std::vector<T> >()) {}
  explicit SharedVector(int n) : d_(std::make_shared<std::vector<T> >(n < 0 ? 0 : n)) {}
  explicit SharedVector(unsigned n) : d_(std::make_shared<std::vector<T> >(n)) {}
  explicit SharedVector(long n) : d_(std::make_shared<std::vector<T> >(n < 0 ? 0 : n)) {}
  explicit SharedVector(unsigned long n) : d_(std::make_shared<std::vector<T> >(n)) {}
  template <typename U>
  SharedVector(const std::vector<U>& v) : d_(std::make_shared<std::vector<T> >(v.begin(), v.end())) {}
  template <typename U>
  SharedVector(const SharedVector<U>& v) : d_(std::make_shared<std::vector<T> >(v.begin(), v.end())) {}
  SharedVector(const SharedVector& v) : d_(v.d_) {}
  SharedVector& operator=(const SharedVector& v) { d_ = v.d_; return *this; }
  static SharedVector create(T a) { SharedVector r(1); r[0] = a; return r; }
  static SharedVector create(T a, T b) { SharedVector r(2); r[0] = a; r[1] = b; return r; }
  static SharedVector create(T a, T b, T c) { SharedVector r(3); r[0] = a; r[1] = b; r[2] = c; return r; }
  unsigned size() const { return (unsigned)d_->size(); }
  unsigned length() const { return size(); }
  T& operator[](long i) { return (*d_)[i]; }
  const T& operator[](long i) const { return (*d_)[i]; }
  T& operator()(long i) { return (*d_)[i]; }
  T* begin() { return d_->data(); }
  T* end() { return d_->data() + d_->size(); }
  const T* begin() const { return d_->data(); }
  const T* end() const { return d_->data() + d_->size(); }
  void fill(T v) { std::fill(d_->begin(), d_->end(), v); }

 private:
  std::shared_ptr<std::vector<T> > d_;
};
typedef SharedVector<double> NumericVector;
typedef SharedVector<int> IntegerVector;
typedef SharedVector<int> LogicalVector;
typedef SharedVector<std::string> CharacterVector;

/* column-major, as R stores a matrix */
class NumericMatrix {
 public:
  typedef double* iterator;
  NumericMatrix() : nr_(0), nc_(0), d_(0) {}
  template <typename A, typename B>
  NumericMatrix(A nr, B nc) : nr_((int)nr), nc_((int)nc), d_((long)nr * (long)nc) {}
  int nrow() const { return nr_; }
  int ncol() const { return nc_; }
  double& operator()(long i, long j) { return d_[j * nr_ + i]; }
  double operator()(long i, long j) const { return d_[j * nr_ + i]; }
  double* begin() { return d_.begin(); }
  double* end() { return d_.end(); }
  unsigned size() const { return d_.size(); }

 private:
  int nr_, nc_;
  NumericVector d_;
};

class List;

/* one R value: the tagged union behind a list element or an attribute */
struct Value {
  enum Kind { NIL, REAL, INT, LGL, STR, NUMVEC, INTVEC, NUMMAT, LIST } kind;
  double real;
  long integer;
  std::string str;
  NumericVector numvec;
  IntegerVector intvec;
  NumericMatrix nummat;
  std::shared_ptr<List> list;
  Value() : kind(NIL), real(0), integer(0) {}
  Value(double x) : kind(REAL), real(x), integer((long)x) {}
  Value(float x) : kind(REAL), real(x), integer((long)x) {}
  Value(int x) : kind(INT), real(x), integer(x) {}
  Value(unsigned x) : kind(INT), real(x), integer(x) {}
  Value(long x) : kind(INT), real((double)x), integer(x) {}
  Value(unsigned long x) : kind(INT), real((double)x), integer((long)x) {}
  Value(bool x) : kind(LGL), real(x), integer(x) {}
  Value(const char* s) : kind(STR), real(0), integer(0), str(s) {}
  Value(const std::string& s) : kind(STR), real(0), integer(0), str(s) {}
  Value(const NumericVector& v) : kind(NUMVEC), real(0), integer(0), numvec(v) {}
  Value(const IntegerVector& v) : kind(INTVEC), real(0), integer(0), intvec(v) {}
  Value(const std::vector<double>& v) : kind(NUMVEC), real(0), integer(0), numvec(v) {}
  Value(const std::vector<int>& v) : kind(INTVEC), real(0), integer(0), intvec(v) {}
  Value(const NumericMatrix& m) : kind(NUMMAT), real(0), integer(0), nummat(m) {}
  Value(const List& l);
  double as_real() const {
    if (kind == NUMVEC && numvec.size() > 0) return numvec[0];
    if (kind == INTVEC && intvec.size() > 0) return intvec[0];
    if (kind == INT || kind == LGL) return (double)integer;
    if (kind != REAL) stop("not a number");
    return real;
  }
};

/* what list["name"], list[i] and list.attr("name") give: converts out, assigns in */
class Proxy {
 public:
  explicit Proxy(Value& v) : v_(v) {}
  template <typename T>
  Proxy& operator=(const T& x) { v_ = Value(x); return *this; }
  Proxy& operator=(const Proxy& o) { v_ = o.v_; return *this; }
  operator double() const { return v_.as_real(); }
  operator int() const { return (int)v_.as_real(); }
  operator unsigned() const { return (unsigned)v_.as_real(); }
  operator bool() const { return v_.as_real() != 0.0; }
  operator std::string() const {
    if (v_.kind != Value::STR) stop("not a string");
    return v_.str;
  }
  operator NumericVector() const {
    if (v_.kind == Value::NUMVEC) return v_.numvec;
    if (v_.kind == Value::INTVEC) return NumericVector(v_.intvec);
    if (v_.kind == Value::NUMMAT) stop("matrix where a vector is expected");
    return NumericVector::create(v_.as_real());
  }
  operator IntegerVector() const {
    if (v_.kind == Value::INTVEC) return v_.intvec;
    if (v_.kind == Value::NUMVEC) return IntegerVector(v_.numvec);
    return IntegerVector::create((int)v_.as_real());
  }
  operator NumericMatrix() const {
    if (v_.kind != Value::NUMMAT) stop("not a matrix");
    return v_.nummat;
  }
  operator List() const;
  operator SEXP() const { return 0; }

 private:
  Value& v_;
};

struct NamedValue {
  std::string name;
  Value value;
};
class Named {
 public:
  explicit Named(const std::string& n) : name_(n) {}
  template <typename T>
  NamedValue operator=(const T& x) const { NamedValue r; r.name = name_; r.value = Value(x); return r; }

 private:
  std::string name_;
};
struct NamedPlaceHolder {
  Named operator[](const std::string& n) const { return Named(n); }
};
static const NamedPlaceHolder _ = NamedPlaceHolder();

class List {
 public:
  List() : d_(std::make_shared<Data>()) {}
  explicit List(int n) : d_(std::make_shared<Data>()) { d_->names.resize(n); d_->values.resize(n); }
  unsigned size() const { return (unsigned)d_->values.size(); }
  Proxy operator[](const char* name) { return Proxy(slot(d_->names, d_->values, name)); }
  Proxy operator[](const std::string& name) { return Proxy(slot(d_->names, d_->values, name)); }
  Proxy operator[](int i) {
    if (i < 0 || (size_t)i >= d_->values.size()) stop("list index out of range");
    return Proxy(d_->values[i]);
  }
  Proxy attr(const std::string& name) { return Proxy(slot(d_->attr_names, d_->attr_values, name)); }
  static List create() { return List(); }
  template <typename... Rest>
  static List create(const NamedValue& first, const Rest&... rest) {
    List l;
    l.push(first, rest...);
    return l;
  }

 private:
  struct Data {
    std::vector<std::string> names, attr_names;
    std::vector<Value> values, attr_values;
  };
  static Value& slot(std::vector<std::string>& names, std::vector<Value>& values, const std::string& name) {
    for (size_t i = 0; i < names.size(); ++i)
      if (names[i] == name) return values[i];
    names.push_back(name);
    values.push_back(Value());
    return values.back();
  }
  void push() {}
  template <typename... Rest>
  void push(const NamedValue& first, const Rest&... rest) {
    d_->names.push_back(first.name);
    d_->values.push_back(first.value);
    push(rest...);
  }
  std::shared_ptr<Data> d_;
};

inline Value::Value(const List& l) : kind(LIST), real(0), integer(0), list(std::make_shared<List>(l)) {}
inline Proxy::operator List() const {
  if (v_.kind != Value::LIST) stop("not a list");
  return *v_.list;
}

template <typename T>
T as(const Proxy& p) { return p.operator T(); }
template <typename T>
T as(const T& x) { return x; }

class RNGScope {};

}  // namespace Rcpp

#endif
