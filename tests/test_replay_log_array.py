"""CPU: replay.log_array — the [S,N,T1+1,6] log both evaluators attach to the engine, from per-scene gt_data_dicts."""
import numpy as np

from helpers import cfg_of
from ctrlsim_amd import replay, scenarios, spec


def test_log_array_truncates_pads_and_takes_the_length_from_the_last_column():
    T1 = 4
    rs = np.random.RandomState(3)
    long_ = rs.uniform(1, 2, (T1 + 4, 8))                  # longer than T1 + 1 rows, 8 columns: the length is the LAST one
    short = rs.uniform(1, 2, (2, 6))
    short[:, 4] = 1.0
    exact = rs.uniform(1, 2, (T1 + 1, 7)).tolist()         # (a list of rows, as a loader may hand it over)
    log = replay.log_array([{0: {"traj": long_}, 1: {"traj": short}, 2: {"traj": exact}}, {v: {"traj": short} for v in range(3)}], 3, T1)
    assert log.shape == (2, 3, T1 + 1, 6) and log.dtype == np.float64
    assert np.array_equal(log[0, 0, :, :5], long_[:T1 + 1, :5]) and np.array_equal(log[0, 0, :, 5], long_[:T1 + 1, 7])
    assert np.array_equal(log[0, 1, :2, :5], short[:, :5]) and np.array_equal(log[0, 1, :2, 5], short[:, 5])
    assert (log[0, 1, 2:] == 0).all()                      # past the end: zero rows, existence 0
    assert np.array_equal(log[0, 2, :, 5], np.array(exact)[:, 6]) and np.array_equal(log[0, 2, :, :5], np.array(exact)[:, :5])
    assert np.array_equal(log[1], np.stack([log[0, 1]] * 3))
    # the latch reads a padded vehicle as gone from the row its log ends at
    assert np.array_equal(replay.latch_all(log, T1)[0, 1], [1, 1, 0, 0])


def test_log_array_equals_the_evaluators_expression_on_a_standin_log():
    cfg = cfg_of("loop")
    T, N = cfg.nocturne.steps, 6
    scn = scenarios.make_scenario(5, 0, n_agents=N, n_polylines=14, n_points=spec.Dims(cfg).NP, extent=40.0)
    gtd = scenarios.standin_log(scn, T, cfg.nocturne.dt)
    T1 = T + 1
    gt = np.zeros((1, N, T1 + 1, 6))                       # PolicyEvaluator._roll_batch before log_array
    for v in range(N):
        tr = np.asarray(gtd[v]["traj"], np.float64)
        n = min(len(tr), T1 + 1)
        gt[0, v, :n, :5] = tr[:n, :5]
        gt[0, v, :n, 5] = tr[:n, -1]
    log = replay.log_array([gtd], N, T1)
    assert np.array_equal(log, gt) and (log[0, :, :T1, 4] == 1).all() and (log[0, :, T1] == 0).all()
    assert np.array_equal(log[0, :, :T1], np.stack([gtd[v]["traj"] for v in range(N)]))
