"""-m gpu: ekf_batch_device_bytes / ekf_device_bytes are the exact sum of the handle's live device allocations (the ledger
of ekf_device_mem.hpp): what is freed leaves the figure, what is regrown counts once, and the delayed mode's buffers are in
it.  The sizes are restated here from the requests of the entry points, never read back from the library."""
import numpy as np
import pytest

from ekf_slam_ml_amd import synth

pytestmark = pytest.mark.gpu

B, N_LM = 2, 4


def _known_log(T, vmax=2):
    return synth.make_known_log(synth.SimConfig(n=N_LM, steps=T, filters=B, seed=91, half_extent=1.0, min_spacing=0.3,
                                                max_visible_dis=1e9, vmax=vmax))


def _known_log_bytes(T, vmax, B=B, n=N_LM):
    """what ekf_batch_upload_known_log requests: twist [T][B][2] f64, lm_idx [T][B][vmax] i32, z_xy [T][B][vmax][2] f64,
    init_xy [B][2n] f64, each at least one element"""
    n_lm = T * B * vmax
    return 8 * max(T * B * 2, 1) + 4 * max(n_lm, 1) + 8 * max(2 * n_lm, 1) + 8 * max(B * 2 * n, 1)


def _unknown_log_bytes(T, jmax, B=B):
    """what ekf_batch_upload_unknown_log requests: twist [T][B][2] f64, count [T][B] i32, meas_xy [T][B][jmax][2] f64,
    decisions [T][B][jmax] i32"""
    n_ct = T * B
    return 8 * T * B * 2 + 4 * n_ct + 8 * max(n_ct * jmax * 2, 1) + 4 * max(n_ct * jmax, 1)


def test_update_mode_round_trip_leaves_the_figure(hip):
    bt = hip.BatchEKF(B, N_LM)
    before = bt.device_bytes()
    bt.set_update_mode(4)
    ld = hip.leading_dimension(N_LM)
    # the pending factors U, V [B][2 * 4][ld] and the second state buffer [B][ld]
    assert bt.device_bytes() - before == 8 * (2 * B * 8 * ld + B * ld)
    bt.set_update_mode(0)
    assert bt.device_bytes() == before
    bt.close()


def test_known_logs_count_once_and_leave_when_replaced(hip):
    bt = hip.BatchEKF(B, N_LM)
    empty = bt.device_bytes()
    log4, log2 = _known_log(4), _known_log(2)
    vmax = log4.lm_idx.shape[2]
    bt.upload_known_log(log4.twist, log4.lm_idx, log4.z_xy, log4.init_xy)
    first = bt.device_bytes()
    assert first - empty == _known_log_bytes(4, vmax)
    bt.upload_known_log(log4.twist, log4.lm_idx, log4.z_xy, log4.init_xy)
    assert bt.device_bytes() == first
    bt.upload_known_log(log2.twist, log2.lm_idx, log2.z_xy, log2.init_xy)
    assert log2.lm_idx.shape[2] == vmax
    shorter = bt.device_bytes()
    assert shorter < first and first - shorter == _known_log_bytes(4, vmax) - _known_log_bytes(2, vmax)
    bt.run_known()
    bt.close()


def test_unknown_run_with_a_wider_log_adds_the_growth_only(hip):
    """a pool's readings live in its log: 64 -> 128 reading slots per step change the figure by the growth of the log's
    buffers (whatever a first run allocates lazily is there before both measurements)"""
    T = 2
    rng = np.random.default_rng(5)
    world = np.array([[0.5, 0.2], [0.4, -0.3], [-0.3, 0.4], [-0.4, -0.4]])
    twist = np.tile([0.01, 0.02], (T, B, 1))
    figures = {}
    bt = hip.BatchEKF(B, N_LM)
    for jmax in (64, 128):
        count = np.full((T, B), 3, dtype=np.int32)
        meas = np.zeros((T, B, jmax, 2))
        meas[:, :, :3] = world[:3] + 1e-3 * rng.standard_normal((T, B, 3, 2))
        bt.reset()
        bt.upload_unknown_log(twist, count, meas)
        st = bt.run_unknown()
        assert st["filter_steps"] == B * T
        figures[jmax] = bt.device_bytes()
    bt.close()
    assert figures[128] - figures[64] == _unknown_log_bytes(T, 128) - _unknown_log_bytes(T, 64)


def test_measurement_capacity_64_to_128_adds_the_growth_only(hip):
    """the measurement capacity belongs to the single filter's data_association(): readings [cap][2] f64 and the block
    [record | record | decisions[cap]] regrow from 64 to 128 -- the figure moves by the growth, not by the new sizes"""
    f = hip.EKF_SLAM(N_LM)
    world = np.array([[0.5, 0.2], [0.4, -0.3], [-0.3, 0.4], [-0.4, -0.4]])
    known = np.zeros(N_LM, dtype=np.uint8)
    f.data_association(world, known)                    # capacity 64
    at64 = f.device_bytes()
    f.data_association(np.tile(world, (16, 1)), known)    # 64 readings: fits
    assert f.device_bytes() == at64
    assoc = f.data_association(np.tile(world, (17, 1))[:65], known)   # 65 readings: capacity 128
    assert assoc.shape == (65,)
    assert f.device_bytes() - at64 == (128 - 64) * 2 * 8 + (128 - 64) * 4
    f.close()
