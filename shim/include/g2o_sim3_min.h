// g2o_sim3_min.h -- the slice of g2o::Sim3 (Thirdparty/g2o/g2o/types/sim3.h:41-292) a caller of
// Optimizer::OptimizeSim3 touches, without g2o or Eigen, in the spirit of opencv_min.hpp: the
// constructor from a rotation matrix, a translation and a scale, rotation(), translation(), scale(),
// operator*, inverse() and map().  The arithmetic is written out in the operation order the library's
// kernel and the tests' restatement use (Eigen's matrix -> quaternion conversion, quaternion product
// and _transformVector); build callers with -ffp-contract=off if their Sim3 values are to match a
// restatement bit for bit.  Like the reference's Sim3 nothing here normalises the quaternion.
#pragma once
#include <array>
#include <cmath>

namespace g2o {

typedef std::array<double, 3> Vector3d;

struct Matrix3d {  // row-major
  std::array<double, 9> m{};
  double& operator()(int r, int c) { return m[3 * r + c]; }
  const double& operator()(int r, int c) const { return m[3 * r + c]; }
};

struct Quaterniond {
  double mx = 0, my = 0, mz = 0, mw = 1;
  Quaterniond() = default;
  Quaterniond(double w, double x, double y, double z) : mx(x), my(y), mz(z), mw(w) {}  // Eigen's argument order
  explicit Quaterniond(const Matrix3d& R) {  // Eigen quaternionbase_assign_impl<Matrix3d>
    const std::array<double, 9>& m = R.m;
    double t = m[0] + m[4] + m[8];
    if (t > 0) {
      t = std::sqrt(t + 1.0);
      mw = 0.5 * t;
      t = 0.5 / t;
      mx = (m[7] - m[5]) * t;
      my = (m[2] - m[6]) * t;
      mz = (m[3] - m[1]) * t;
    } else {
      int i = 0;
      if (m[4] > m[0]) i = 1;
      if (m[8] > m[4 * i]) i = 2;
      const int j = (i + 1) % 3, k = (j + 1) % 3;
      double c[3];
      t = std::sqrt(m[4 * i] - m[4 * j] - m[4 * k] + 1.0);
      c[i] = 0.5 * t;
      t = 0.5 / t;
      mw = (m[3 * k + j] - m[3 * j + k]) * t;
      c[j] = (m[3 * j + i] + m[3 * i + j]) * t;
      c[k] = (m[3 * k + i] + m[3 * i + k]) * t;
      mx = c[0];
      my = c[1];
      mz = c[2];
    }
  }
  double x() const { return mx; }
  double y() const { return my; }
  double z() const { return mz; }
  double w() const { return mw; }
  Quaterniond conjugate() const { return Quaterniond(mw, -mx, -my, -mz); }
  Quaterniond operator*(const Quaterniond& b) const {
    const Quaterniond& a = *this;
    return Quaterniond(a.mw * b.mw - (a.mx * b.mx + a.my * b.my + a.mz * b.mz),
                       a.mw * b.mx + b.mw * a.mx + (a.my * b.mz - a.mz * b.my),
                       a.mw * b.my + b.mw * a.my + (a.mz * b.mx - a.mx * b.mz),
                       a.mw * b.mz + b.mw * a.mz + (a.mx * b.my - a.my * b.mx));
  }
  Vector3d operator*(const Vector3d& v) const {  // _transformVector
    Vector3d uv = {my * v[2] - mz * v[1], mz * v[0] - mx * v[2], mx * v[1] - my * v[0]};
    uv[0] += uv[0];
    uv[1] += uv[1];
    uv[2] += uv[2];
    const Vector3d c = {my * uv[2] - mz * uv[1], mz * uv[0] - mx * uv[2], mx * uv[1] - my * uv[0]};
    return Vector3d{v[0] + mw * uv[0] + c[0], v[1] + mw * uv[1] + c[1], v[2] + mw * uv[2] + c[2]};
  }
  Matrix3d toRotationMatrix() const {
    const double tx = 2 * mx, ty = 2 * my, tz = 2 * mz;
    const double twx = tx * mw, twy = ty * mw, twz = tz * mw;
    const double txx = tx * mx, txy = ty * mx, txz = tz * mx;
    const double tyy = ty * my, tyz = tz * my, tzz = tz * mz;
    Matrix3d R;
    R.m = {1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz), tyz - twx,
           txz - twy, tyz + twx, 1 - (txx + tyy)};
    return R;
  }
};

struct Sim3 {
 protected:
  Quaterniond r;
  Vector3d t;
  double s;

 public:
  Sim3() : t{0., 0., 0.}, s(1.) {}
  Sim3(const Quaterniond& r_, const Vector3d& t_, double s_) : r(r_), t(t_), s(s_) {}
  Sim3(const Matrix3d& R, const Vector3d& t_, double s_) : r(Quaterniond(R)), t(t_), s(s_) {}

  Vector3d map(const Vector3d& xyz) const {
    const Vector3d p = r * xyz;
    return Vector3d{s * p[0] + t[0], s * p[1] + t[1], s * p[2] + t[2]};
  }
  Sim3 inverse() const {
    const double c = -1. / s;
    return Sim3(r.conjugate(), r.conjugate() * Vector3d{c * t[0], c * t[1], c * t[2]}, 1. / s);
  }
  Sim3 operator*(const Sim3& other) const {
    Sim3 ret;
    ret.r = r * other.r;
    const Vector3d p = r * other.t;
    ret.t = Vector3d{s * p[0] + t[0], s * p[1] + t[1], s * p[2] + t[2]};
    ret.s = s * other.s;
    return ret;
  }
  const Vector3d& translation() const { return t; }
  Vector3d& translation() { return t; }
  const Quaterniond& rotation() const { return r; }
  Quaterniond& rotation() { return r; }
  const double& scale() const { return s; }
  double& scale() { return s; }
};

}  // namespace g2o
