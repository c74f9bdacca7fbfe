// oracle/ref_ekf_shim.cpp -- TEST INFRASTRUCTURE ONLY.
// extern "C" doors into the reference's OWN rigid2d::EKF_SLAM (rigid2d/src/ekf_slam.cpp), which oracle/Makefile
// compiles where it lies, against the tests-only Armadillo subset tests/cpp/arma_double/armadillo, into
// oracle/_ref/libekf_slam_ref.so.  oracle/binding.py's RefEKF duck-types OracleEKF over it, so the restatements
// (ekf_oracle.c DENSE / STRUCTURED, np_restatement.py) and the HIP kernels are checked against the reference itself.
//
// The class keeps state / sigma / landmark_init_flag private and has no setters; they are reached through the
// explicit-instantiation member-pointer idiom (access checks do not apply to the template arguments of an explicit
// instantiation, [temp.spec]/6).  The reference prints to std::cout on every association; each call runs with
// std::cout on a null buffer.  Every door returns 0 on success and 1 when the reference (or the Armadillo subset's
// bounds / shape checks) threw; ekfr_last_error() then holds the message.
#include <cstring>
#include <iostream>
#include <streambuf>
#include <string>
#include <vector>

#include "rigid2d/ekf_slam.hpp"

namespace {

template <class Tag, typename Tag::type M>
struct Rob {
    friend typename Tag::type get(Tag) { return M; }
};
struct StateTag { typedef arma::mat rigid2d::EKF_SLAM::*type; friend type get(StateTag); };
struct SigmaTag { typedef arma::mat rigid2d::EKF_SLAM::*type; friend type get(SigmaTag); };
struct NTag { typedef int rigid2d::EKF_SLAM::*type; friend type get(NTag); };
struct FlagTag { typedef bool rigid2d::EKF_SLAM::*type; friend type get(FlagTag); };
struct MahaTag { typedef double (rigid2d::EKF_SLAM::*type)(rigid2d::Vector2D, int); friend type get(MahaTag); };

}  // namespace

template struct Rob<StateTag, &rigid2d::EKF_SLAM::state>;
template struct Rob<SigmaTag, &rigid2d::EKF_SLAM::sigma>;
template struct Rob<NTag, &rigid2d::EKF_SLAM::n>;
template struct Rob<FlagTag, &rigid2d::EKF_SLAM::landmark_init_flag>;
template struct Rob<MahaTag, &rigid2d::EKF_SLAM::calculate_maha_dis>;

namespace {

struct NullBuf : std::streambuf {
    int overflow(int c) override { return traits_type::not_eof(c); }
};

// std::cout -> a null buffer for one call, restored on every exit path
struct Quiet {
    NullBuf sink;
    std::streambuf* old;
    Quiet() : old(std::cout.rdbuf(&sink)) {}
    ~Quiet() { std::cout.rdbuf(old); }
};

thread_local std::string last_error;

template <class F>
int guarded(F f) {
    Quiet q;
    try {
        f();
        return 0;
    } catch (const std::exception& e) {
        last_error = e.what();
    } catch (...) {
        last_error = "unknown exception";
    }
    return 1;
}

rigid2d::EKF_SLAM& ekf(void* h) { return *static_cast<rigid2d::EKF_SLAM*>(h); }
int n_of(void* h) { return ekf(h).*get(NTag()); }

}  // namespace

extern "C" {

const char* ekfr_last_error() { return last_error.c_str(); }

// ekf_slam.cpp:27-53
void* ekfr_create(int n) {
    rigid2d::EKF_SLAM* p = nullptr;
    if (guarded([&] { p = new rigid2d::EKF_SLAM(n); })) return nullptr;
    return p;
}

void ekfr_destroy(void* h) { delete static_cast<rigid2d::EKF_SLAM*>(h); }

// ekf_slam.cpp:55-106; the node builds the twist as Twist2D(angular, Vector2D{x, 0})
int ekfr_prediction(void* h, double dtheta, double dx) {
    return guarded([&] { ekf(h).prediction(rigid2d::Twist2D(dtheta, rigid2d::Vector2D{dx, 0.0})); });
}

// ekf_slam.cpp:108-197: sensor_xy[2n] (x0, y0, x1, ...), visible[n]; known_list is not read by measurement()
int ekfr_measurement(void* h, const double* sensor_xy, const unsigned char* visible) {
    return guarded([&] {
        const int n = n_of(h);
        arma::mat s(sensor_xy, 2 * n, 1);
        std::vector<bool> vis(n), known(n, false);
        for (int i = 0; i < n; i++) vis[i] = visible[i] != 0;
        ekf(h).measurement(s, vis, known);
    });
}

// ekf_slam.cpp:278-402: meas_xy[2J]; known[n] in / out
int ekfr_data_association(void* h, const double* meas_xy, int J, unsigned char* known) {
    return guarded([&] {
        const int n = n_of(h);
        std::vector<rigid2d::Vector2D> m(J);
        for (int j = 0; j < J; j++) m[j] = rigid2d::Vector2D{meas_xy[2 * j], meas_xy[2 * j + 1]};
        std::vector<bool> kl(n);
        for (int i = 0; i < n; i++) kl[i] = known[i] != 0;
        ekf(h).data_association(m, kl);
        for (int i = 0; i < n; i++) known[i] = kl[i] ? 1 : 0;
    });
}

// ekf_slam.cpp:217-276
int ekfr_maha(void* h, double mx, double my, int i, double* out) {
    return guarded([&] { *out = (ekf(h).*get(MahaTag()))(rigid2d::Vector2D{mx, my}, i); });
}

int ekfr_dim(void* h) { return 3 + 2 * n_of(h); }

int ekfr_get_state(void* h, double* out) {
    return guarded([&] {
        const arma::mat& s = ekf(h).*get(StateTag());
        std::memcpy(out, s.memptr(), sizeof(double) * s.n_elem);
    });
}

int ekfr_set_state(void* h, const double* in) {
    return guarded([&] {
        arma::mat& s = ekf(h).*get(StateTag());
        s = arma::mat(in, s.n_rows, 1);
    });
}

// covariance as ROW-major N x N (oracle/ekf_oracle.c's layout); the reference stores it column-major
int ekfr_get_cov(void* h, double* out) {
    return guarded([&] {
        const arma::mat& S = ekf(h).*get(SigmaTag());
        for (arma::uword r = 0; r < S.n_rows; r++)
            for (arma::uword c = 0; c < S.n_cols; c++) out[r * S.n_cols + c] = S(r, c);
    });
}

int ekfr_set_cov(void* h, const double* in) {
    return guarded([&] {
        arma::mat& S = ekf(h).*get(SigmaTag());
        for (arma::uword r = 0; r < S.n_rows; r++)
            for (arma::uword c = 0; c < S.n_cols; c++) S(r, c) = in[r * S.n_cols + c];
    });
}

int ekfr_get_init_flag(void* h) { return (ekf(h).*get(FlagTag())) ? 1 : 0; }
void ekfr_set_init_flag(void* h, int f) { ekf(h).*get(FlagTag()) = f != 0; }

}
