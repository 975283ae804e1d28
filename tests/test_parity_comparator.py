"""parity.compare can fail: the oracle against a copy of itself passes with deviation 0, and the same copy with one planted defect is rejected, for each of the
algorithms the geometry sweep covers (CPU only: no deliberately wrong kernel is built).  RLEPSO, whose comparison runs generation by generation, also gets a stagnation
counter that is off without a near-tie behind it and a wrong __reinit flag."""
import numpy as np
import pytest

import parity
from helpers import problems

ALGOS = ('rlepso', 'lde', 'gleet', 'rlpso', 'qlpso', 'de', 'pso')
DEFECTS = ('coordinate', 'pbest', 'cost_len', 'curve')
NP, D = 5, 3
BUDGET = (3 * NP + 17, (3 * NP + 17) // 5, 5)


def _records(name):
    steps = 2 * NP + 17 if name in parity.PER_PARTICLE else 6
    acts = parity.actions_for(name, steps, 4, NP)
    return [parity.oracle_record(name, problems('bbob', D)[f], NP, D, BUDGET, 7 + k, None if acts is None else acts[:, k], steps)
            for k, f in enumerate((1, 3, 10, 15))]


@pytest.mark.parametrize('name', ALGOS)
def test_comparator_accepts_the_oracle_and_rejects_every_planted_defect(name):
    recs = _records(name)
    for k, rec in enumerate(recs):
        assert rec['done'][-1]
        st = parity.compare(name, rec, rec, f'{name} #{k}', ledger=[])
        assert st and max(st.values()) == 0
    for defect in DEFECTS:
        planted = [(k, parity.plant(rec, defect)) for k, rec in enumerate(recs)]
        planted = [(k, bad) for k, bad in planted if bad is not None]
        assert planted, (name, defect, 'no record offers a place for this defect')
        for k, bad in planted:
            with pytest.raises(AssertionError):
                parity.compare(name, bad, recs[k], f'{name} #{k} {defect}', ledger=[])


@pytest.mark.parametrize('defect', ['pni', 'reinit', 'fes'])
def test_comparator_rejects_rlepso_bookkeeping_defects(defect):
    for k, rec in enumerate(_records('rlepso')):
        bad = parity.plant(rec, defect)
        with pytest.raises(AssertionError):
            parity.compare('rlepso', bad, rec, f'rlepso #{k} {defect}', ledger=[])
