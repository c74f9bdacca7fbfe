"""CPU: the drop-in files shim/rigid2d/{include/rigid2d/ekf_slam.hpp, src/ekf_slam.cpp} really
compile -- against the reference's REAL rigid2d.hpp (rigid2d::Twist2D / Vector2D), by build() into oracle/_ref/ where the
reference sources lie at build time, and against a matrix type with the members of arma::Mat<double>
(tests/cpp/arma_double/armadillo, a tests-only double: Armadillo is not a dependency of this project).  A compile check of
OUR forwarding code.  Parity is pinned elsewhere: tests/test_reference_ekf.py builds the reference's own ekf_slam.cpp
against an extended form of the same double.
Reference surface: rigid2d/include/rigid2d/ekf_slam.hpp:19-57; callers nuslam/src/slam.cpp:213,428,433-434."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_OBJ = os.path.join(ROOT, "oracle", "_ref")


def _gxx(args, **kw):
    return subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + args, capture_output=True, text=True, **kw)


def _ref_object(name):
    """oracle/_ref/<name>: compiled by build() (oracle/Makefile, target `ref`) against the reference's real rigid2d.hpp
    with -Wall -Werror, where the reference sources lie at build time."""
    path = os.path.join(REF_OBJ, name)
    if not os.path.exists(path):
        pytest.skip(f"oracle/_ref/{name} not built (reference sources absent at build time)")
    return path


def _nm(path, *flags):
    return subprocess.run(["nm", "-C"] + list(flags) + [path], capture_output=True, text=True, check=True).stdout


def test_shim_compiles_against_the_real_rigid2d_headers():
    obj = _ref_object("ekf_slam_shim.o")
    # the object defines exactly the reference's public member functions
    syms = _nm(obj, "--defined-only")
    for want in ["rigid2d::EKF_SLAM::EKF_SLAM()", "rigid2d::EKF_SLAM::EKF_SLAM(int)",
                 "rigid2d::EKF_SLAM::prediction(rigid2d::Twist2D const&)",
                 "rigid2d::EKF_SLAM::measurement(arma::mat, std::vector<bool",
                 "rigid2d::EKF_SLAM::data_association(std::vector<rigid2d::Vector2D",
                 "rigid2d::EKF_SLAM::getStateX()", "rigid2d::EKF_SLAM::getStateY()",
                 "rigid2d::EKF_SLAM::getStateTheta()", "rigid2d::EKF_SLAM::getStateLandmark()"]:
        assert want in syms, f"shim object lacks {want}"


def test_a_caller_like_nuslam_compiles_against_the_shim_header():
    """slam.cpp's usage pattern (tests/cpp/nuslam_caller.cpp): by-value member, copy-assignment from a temporary
    (:213,428), bare `mat` (:217,380) -- and every shim member it calls is one the shim object defines."""
    caller = _ref_object("nuslam_caller.o")
    shim = _ref_object("ekf_slam_shim.o")
    defined = {l.split(" ", 2)[2] for l in _nm(shim, "--defined-only").splitlines() if l.count(" ") >= 2}
    called = [l.split("U ", 1)[1] for l in _nm(caller, "--undefined-only").splitlines() if "rigid2d::EKF_SLAM::" in l]
    assert len(called) >= 8, called
    for sym in called:
        assert sym in defined, f"the caller needs {sym}, which the shim does not define"


def test_mirror_accepts_a_type_with_both_arma_and_std_spellings(tmp_path):
    """Round-1 defect: detail::size_of / data_of were unranked SFINAE pairs, ambiguous for a type exposing memptr(),
    n_elem AND size()/data() -- which arma::Mat does.  Needs no reference header."""
    src = tmp_path / "both.cpp"
    src.write_text('''
#include "ekf_slam_ml_amd/host/ekf_slam.hpp"
struct Both {                       // every spelling at once
    unsigned long long n_elem = 0;
    const double* memptr() const { return nullptr; }
    const double* data() const { return nullptr; }
    unsigned long long size() const { return n_elem; }
};
struct Twist { double angular() const { return 0; } double linearX() const { return 0; } };
void use(ekfslam::EKF_SLAM& f, Both m, std::vector<double> v, std::vector<bool> b) {
    f.measurement(m, b, b);         // arma-like
    f.measurement(v, b, b);         // std::vector
    f.prediction(Twist{});
    static_assert(sizeof(ekfslam::detail::size_of(m)) == sizeof(size_t), "");
}
int main() { return 0; }
''')
    r = _gxx(["-fsyntax-only", "-I" + ROOT, str(src)])
    assert r.returncode == 0, r.stderr
