"""GPU tests of the seeded combination sweep (tests/rad_pass_sweep.py): every family x seed x orientation of the seven record passes,
from host bytes, compared exactly with the family's existing judge.  tests/test_rad_pass_sweep_cpu.py shows what the seeds reach."""
import numpy as np
import pytest

import rad_pass_calls as P
import rad_pass_sweep as S
from util import pkg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def q():
    cfg = pkg.WorkerConfig.for_resolution("cr-like", num_genes=1, num_rows=1)
    qq = pkg.Quantifier(cfg, np.zeros(1, np.uint32), device=0)
    yield qq
    qq.close()


@pytest.mark.parametrize("family", S.FAMILIES)
def test_every_seed_and_orientation_equals_the_judge(q, family):
    lim = S.LIMITS[family]()
    drawn = compared = 0
    for seed in S.SEEDS[family]:
        c = S.draw(family, seed, lim)
        for ori in S.ORIS[family]:
            drawn += 1
            got = P.run(family, q, c, ori, c["data"], c["off"])
            P.same(family, got, S.want(family, c, ori, lim), c, f"{family} seed {seed} {ori}")
            compared += 1
    assert compared == drawn == 8 * len(S.ORIS[family])
