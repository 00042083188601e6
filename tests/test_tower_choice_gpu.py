"""The rule that tests/test_tower_choice_cpu.py holds to its table is the one the library launches by: az_net_forward on both sides
of three break-points of the table, at the device's CU count, must report the form the table gives (az_net_last_kernel)."""
import numpy as np
import pytest

from azhip.network import ResNetHP, random_params
from test_tower_choice_cpu import at, golden_lines, sweeps

NAMES = {3: "k_tower16<ConnectFour,64,NT=3>", 7: "k_tower16<ConnectFour,64,NT=6>", 16: "k_tower16<ConnectFour,64,NT=11>",
         21: "k_tower16x2<ConnectFour,64>", 32: "k_tower<ConnectFour,64>"}


@pytest.mark.gpu
def test_forward_launches_the_form_of_the_table():
    import azhip
    hp = ResNetHP(num_blocks=2, num_filters=64, num_policy_head_filters=32, num_value_head_filters=32)
    table, _ = sweeps(golden_lines())
    rng = np.random.default_rng(7)
    X = (rng.random((1600, 3, 6, 7)) < 0.3).astype(np.float32)      # (any planes: the outputs are compared among the forms only)
    A = np.ones((1600, 7), dtype=np.float32)
    with azhip.Engine(game=azhip.GAME_CONNECT_FOUR, oracle=azhip.ORACLE_RESNET, num_workers=8, batch_size=8, num_iters_per_turn=8,
                      num_blocks=2, num_filters=64, num_policy_head_filters=32, num_value_head_filters=32) as e:
        e.net_set_params(random_params(azhip.GAME_CONNECT_FOUR, hp, seed=11))
        cu = e.device_info()[1]
        key = "A ConnectFour F=64 bf16=0 groups=1 cu=%d" % cu
        assert key in table, "the table has no sweep at this device's %d CUs" % cu
        points = table[key]
        # the first break-point into each of k_tower, the 11-tile form and the paired form (256 CUs: 513, 769, 1537)
        breaks = [next(n for n, f in points if f == form) for form in (32, 16, 21)]
        assert all(1 < n <= 1600 for n in breaks), breaks
        first = None
        for n in breaks:
            for m in (n - 1, n):
                P, V, _ = e.net_forward(X[:m], A[:m])
                assert e.net_last_kernel() == NAMES[at(points, m)[0]], (m, e.net_last_kernel())
                if first is None:
                    first = (P, V)
                assert np.array_equal(P[:first[0].shape[0]], first[0]) and np.array_equal(V[:first[1].shape[0]], first[1])   # every fp32 form: the same bits
