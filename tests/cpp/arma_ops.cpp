// extern "C" door to single operations of the tests-only Armadillo subset (tests/cpp/arma_double/armadillo), so that
// tests/test_reference_ekf.py can hold each one against NumPy.  Matrices cross the door column-major, as arma stores
// them.  Returns 0 on success, 1 when the operation threw std::logic_error (shape / bounds checks), 2 when it threw
// std::runtime_error (singular inverse).
#include <cstring>
#include <stdexcept>

#include <armadillo>

using arma::mat;
using arma::uword;

enum { OP_MUL, OP_ADD, OP_SUB, OP_SCALE_R, OP_SCALE_L, OP_T, OP_I, OP_ROWS, OP_JOIN_H, OP_JOIN_V, OP_EYE_SIZE, OP_AT,
       OP_EYE_RC };

extern "C" int arma_op(int op, const double* a, int ar, int ac, const double* b, int br, int bc, double s, int i0,
                       int i1, double* out, int* out_rows, int* out_cols) {
    try {
        const mat A(a, ar, ac), B(b, br, bc);
        mat R;
        switch (op) {
            case OP_MUL: R = A * B; break;
            case OP_ADD: R = A + B; break;
            case OP_SUB: R = A - B; break;
            case OP_SCALE_R: R = A * s; break;
            case OP_SCALE_L: R = s * A; break;
            case OP_T: R = A.t(); break;
            case OP_I: R = A.i(); break;
            case OP_ROWS: R = A.rows(i0, i1); break;
            case OP_JOIN_H: R = join_horiz(A, B); break;
            case OP_JOIN_V: R = join_vert(A, B); break;
            case OP_EYE_SIZE: R = eye(size(A)); break;
            case OP_AT: R = mat(1, 1); R(0, 0) = A(i0, i1); break;
            case OP_EYE_RC: R = arma::eye(i0, i1); break;
            default: throw std::logic_error("unknown op");
        }
        *out_rows = (int)R.n_rows;
        *out_cols = (int)R.n_cols;
        if (R.n_elem) std::memcpy(out, R.memptr(), sizeof(double) * R.n_elem);
        return 0;
    } catch (const std::runtime_error&) {
        return 2;
    } catch (const std::logic_error&) {
        return 1;
    }
}

// the reference's row-list construction, mat H = {{...}, {...}} (ekf_slam.cpp's Jacobian blocks)
extern "C" int arma_init_2x3(const double* rowmajor, double* out) {
    const mat H = {{rowmajor[0], rowmajor[1], rowmajor[2]}, {rowmajor[3], rowmajor[4], rowmajor[5]}};
    if (H.n_rows != 2 || H.n_cols != 3) return 1;
    std::memcpy(out, H.memptr(), sizeof(double) * 6);
    return 0;
}
