"""The posterior over orders and the ancestral sampler on their numpy restatement alone
(tests/order_posterior_ref.py), driven by the float64 step distributions of
beam_batch_ref.random_case at H = 16: the invariants the device kernels are then held to
(tests/test_order_posterior_gpu.py), and the proof that the seeds the GPU test uses pass the
sampler's count test on the reference itself.
"""
import itertools

import numpy as np
import pytest

import beam_batch_ref as R
import mlm_mask_ref as M
import order_posterior_ref as P
import order_score_ref as S

H = 16
SAMPLE_CASE = (2, 4, H)       # (B, N, H) of the sampler's count test, CPU and GPU
SAMPLE_S = 4096
SAMPLE_SEEDS = (11, 2024)

_CASES = {}


def case_rows(B, N):
    """(case, [step_rows64 per story], perms [N!][N], float64 NLLs [B][N!]), once per shape."""
    if (B, N) not in _CASES:
        case = R.random_case(B, N, H, R.SEED)
        c64 = P.case64(case)
        rows = [P.step_rows64(c64, b) for b in range(B)]
        perms = P.all_perms(N)
        _CASES[(B, N)] = (case, rows, perms, np.stack([P.nll64(r, perms) for r in rows]))
    return _CASES[(B, N)]


def count_bound(S_, p):
    """5 sigma of a binomial count plus one."""
    return 5.0 * np.sqrt(S_ * p * (1.0 - p)) + 1.0


@pytest.mark.parametrize("N", [1, 2, 3, 5])
def test_pointer_decoder_is_a_distribution_over_permutations(N):
    B = 2
    case, rows, perms, nll = case_rows(B, N)
    assert np.abs(np.exp(-nll).sum(1) - 1.0).max() < 1e-9
    # the float64 NLLs are the reference scorer's (f32 arithmetic) within the project's bound
    _, cand, want = S.ref_nll(B, N, H)
    assert [list(map(int, o)) for o in perms] == cand
    for b in range(B):
        for k in range(len(cand)):
            assert abs(nll[b, k] - float(want[b, k])) < R.bound(float(want[b, k]))


@pytest.mark.parametrize("N", [1, 2, 3, 5])
def test_marginals(N):
    B = 2
    case, rows, perms, nll = case_rows(B, N)
    post = P.posterior_ref(perms, nll.astype(np.float32), 0)
    for b in range(B):
        pos, bef = post["position"][b].astype(np.float64), post["before"][b].astype(np.float64)
        assert np.abs(pos.sum(0) - 1).max() < 1e-6 and np.abs(pos.sum(1) - 1).max() < 1e-6
        off = ~np.eye(N, dtype=bool)
        assert np.abs((bef + bef.T)[off] - 1).max(initial=0) < 1e-6
        assert (np.diag(bef) == 0).all()
        assert abs(float(post["logz"][b])) < 1e-5  # f32 scores: sum exp(-nll) = 1 to their rounding
        if N > 1:
            first = np.exp(-rows[b][()])  # the first step's softmax
            assert np.abs(pos[0] - first).max() < 1e-5
        p = np.exp(-nll[b])
        assert abs(float(post["entropy"][b]) - float(-(p * np.log(p)).sum())) < 1e-5
        assert abs(float(post["map_prob"][b]) - p.max()) < 1e-5
        assert int(post["map_index"][b]) == int(np.argmin(nll[b].astype(np.float32)))


def _brute(perms, position, before):
    """Expected accuracy / tau of every candidate, straight from the definitions."""
    N = perms.shape[1]
    acc, tau = [], []
    for o in perms:
        acc.append(sum(np.float64(position[t, o[t]]) for t in range(N)) / np.float64(N))
        s = np.float64(0)
        for i, j in itertools.combinations(range(N), 2):
            s = s + (np.float64(before[o[i], o[j]]) - np.float64(before[o[j], o[i]]))
        tau.append(s / np.float64(N * (N - 1) // 2) if N > 1 else np.float64(1))
    return np.array(acc), np.array(tau)


@pytest.mark.parametrize("N", [1, 2, 3, 5])
def test_mbr_is_the_brute_force_argmax(N):
    B = 2
    case, rows, perms, nll = case_rows(B, N)
    post = P.posterior_ref(perms, nll.astype(np.float32), 0)
    for b in range(B):
        acc, tau = _brute(perms, post["position"][b], post["before"][b])
        ia, it, im = (int(post[k][b]) for k in ("mbr_acc_index", "mbr_tau_index", "map_index"))
        assert ia == int(np.argmax(acc)) and it == int(np.argmax(tau))
        assert np.float32(acc[ia]) == post["exp_acc"][b] and np.float32(tau[it]) == post["exp_tau"][b]
        assert acc[ia] >= acc[im] and tau[it] >= tau[im]
        # the expectations are cal_result's per-story metrics averaged under p
        p = np.exp(-nll[b])
        o = perms[ia]
        want_acc = sum(p[k] * np.mean(perms[k] == o) for k in range(len(perms)))
        assert abs(acc[ia] - want_acc) < 1e-6
        if N > 1:
            o = perms[it]
            pos = np.argsort(o)
            want_tau = 0.0
            for k, cand in enumerate(perms):  # tau of prediction o against truth cand
                inv = sum(1 for i, j in itertools.combinations(range(N), 2)
                          if pos[cand[i]] > pos[cand[j]])
                want_tau += p[k] * (1 - 2 * inv / (N * (N - 1) / 2))
            assert abs(tau[it] - want_tau) < 1e-6


def test_tie_rules_on_hand_made_scores():
    perms = P.all_perms(3)
    # equal weights: everything ties, the lowest index wins everywhere
    post = P.posterior_ref(perms, np.full((1, 6), 1.5, np.float32), 0)
    assert [int(post[k][0]) for k in P.INT_OUT] == [0, 0, 0]
    assert np.abs(post["position"][0] - 1 / 3).max() < 1e-7
    assert abs(float(post["entropy"][0]) - np.log(6)) < 1e-6
    assert abs(float(post["logz"][0]) - (np.log(6) - 1.5)) < 1e-6
    # -0.0 and +0.0 tie: the lower index is the heaviest
    nll = np.array([[3.0, 0.0, -0.0, 3.0, 3.0, 3.0]], np.float32)
    assert int(P.posterior_ref(perms, nll, 0)["map_index"][0]) == 1
    nll = np.array([[3.0, -0.0, 0.0, 3.0, 3.0, 3.0]], np.float32)
    assert int(P.posterior_ref(perms, nll, 0)["map_index"][0]) == 1
    # +inf rows weigh nothing and are never chosen, whatever their order holds
    nll = np.array([[np.inf, 2.0, np.inf, 2.0, np.inf, np.inf]], np.float32)
    post = P.posterior_ref(perms, nll, 0)
    assert [int(post[k][0]) for k in P.INT_OUT] == [1, 1, 1]
    assert abs(float(post["map_prob"][0]) - 0.5) < 1e-7
    assert post["position"][0][0].tolist() == [0.5, 0.5, 0.0]  # perms 1, 3 = (0,2,1), (1,2,0)
    padded = np.concatenate([perms[[1, 3]], np.full((2, 3), -1)])
    post2 = P.posterior_ref(padded, np.array([[2.0, 2.0, np.inf, np.inf]], np.float32), 0)
    assert np.array_equal(post2["position"], post["position"])
    assert np.array_equal(post2["before"], post["before"])
    # an out-of-range entry or a repeat invalidates a finite-scored candidate
    bad = perms.copy()
    bad[0] = [0, 1, 3]
    bad[1] = [0, 0, 1]
    post = P.posterior_ref(bad, np.zeros((1, 6), np.float32), 0)
    assert int(post["map_index"][0]) == 2 and abs(float(post["logz"][0]) - np.log(4)) < 1e-6
    # a story without a valid candidate
    post = P.posterior_ref(perms, np.full((1, 6), np.inf, np.float32), 0)
    assert [int(post[k][0]) for k in P.INT_OUT] == [-1, -1, -1]
    assert post["logz"][0] == -np.inf and not post["position"].any() and not post["before"].any()
    # uniform mode: a repeated order counts as often as it occurs
    rep = perms[[0, 4, 4, 4]]
    post = P.posterior_ref(rep, np.array([[9.0, 1.0, 2.0, 3.0]], np.float32), 1)
    assert abs(float(post["logz"][0]) - np.log(4)) < 1e-7
    assert post["position"][0][0].tolist() == [0.25, 0.0, 0.75]  # perms[4] = (2, 0, 1)
    assert int(post["map_index"][0]) == 0 and int(post["mbr_acc_index"][0]) == 1


def test_uniforms_are_the_mlm_hash():
    B, S_, N = 3, 64, 5
    u = P.uniforms(B, S_, N, seed=7, stream_id=2)
    h = M.hashes(S_ * (N - 1), 7, 2)[0]
    want = ((h >> np.uint64(8)).astype(np.float64) * 2.0 ** -24).astype(np.float32)
    assert np.array_equal(u[0].reshape(-1), want)
    assert (u >= 0).all() and (u < 1).all()
    assert not np.array_equal(u[0], u[1]) and not np.array_equal(u[1], u[2])
    # a pure function of (story, sample, step): independent of S, B and of where a chunk starts
    assert np.array_equal(P.uniforms(B, 256, N, 7, 2)[:, :64], u)
    assert np.array_equal(P.uniforms(1, 16, N, 7, 2, story0=2, sample0=48)[0], u[2, 48:])
    assert not np.array_equal(P.uniforms(B, S_, N, 8, 2), u)


def test_pick_rule():
    row = -np.log(np.array([0.1, 0.2, np.nan, 0.3, 0.4]))
    row[2] = np.inf  # pointed
    for u, want in ((0.0, 0), (0.0999, 0), (0.1001, 1), (0.2999, 1), (0.3001, 3), (0.5999, 3),
                    (0.6001, 4), (0.99999994, 4)):
        assert P.pick_ref(row, u)[0] == want, u
    assert P.pick_ref(row, 0.3)[1] < 1e-12 and P.pick_ref(row, 0.45)[1] > 0.1
    assert P.pick_ref(np.array([np.inf, 0.0, np.inf]), 0.7)[0] == 1


def test_sampler_counts_match_the_exact_posterior():
    B, N, _ = SAMPLE_CASE
    case, rows, perms, nll = case_rows(B, N)
    index = {tuple(o): k for k, o in enumerate(perms.tolist())}
    for seed in SAMPLE_SEEDS:
        u = P.uniforms(B, SAMPLE_S, N, seed)
        for b in range(B):
            orders = P.sample_ref(rows[b], u[b])
            assert (np.sort(orders, -1) == np.arange(N)).all()
            counts = np.bincount([index[tuple(o)] for o in orders.tolist()], minlength=len(perms))
            p = np.exp(-nll[b])
            worst = np.abs(counts - SAMPLE_S * p) / count_bound(SAMPLE_S, p)
            print(f"seed {seed} story {b}: largest |count - S p| / bound = {worst.max():.3f}")
            assert (worst <= 1.0).all(), (seed, b, counts.tolist())
            # the uniform posterior over the samples estimates the marginals
            est = P.posterior_ref(orders, np.zeros((1, SAMPLE_S), np.float32), 1)
            exact = P.posterior_ref(perms, nll[b:b + 1].astype(np.float32), 0)
            assert np.abs(est["position"] - exact["position"]).max() < 5 * 0.5 / np.sqrt(SAMPLE_S)
