"""accepter._unwrap_accepter and its three readers: the device plan, the
host plan and TemperedSMC object to the same compositions, with the same
exceptions, whatever the order of the layers.  No GPU is used."""
import numpy as np
import pytest

from ip_mcmc_amd import (BoxConstraint, ConstrainAccepter, ConstSteppCNProposer, CountedAccepter, GaussianDistribution,
                         StandardRWAccepter, TemperedSMC, pCNAccepter)
from ip_mcmc_amd._lib import UnsupportedOnDevice
from ip_mcmc_amd.accepter import _unwrap_accepter
from ip_mcmc_amd.hostloop import GenericComposition, HostPlan
from ip_mcmc_amd.sampler import _Plan

PRIOR = GaussianDistribution(np.zeros(2), np.eye(2))
PROPOSER = ConstSteppCNProposer(0.3, PRIOR)


def _phi(u):
    return 0.0


def below(v):
    return bool(np.all(v < 1))


def test_layers_come_outermost_first():
    core = pCNAccepter(_phi)
    inner = CountedAccepter(core)
    con = ConstrainAccepter(inner, BoxConstraint(-1, 1))
    outer = CountedAccepter(con)
    layers, found = _unwrap_accepter(outer)
    assert [id(x) for x in layers] == [id(outer), id(con), id(inner)] and found is core
    assert _unwrap_accepter(core) == ([], core)


def test_core_is_whatever_lies_beneath():
    rw = StandardRWAccepter(_phi, PRIOR)
    assert _unwrap_accepter(CountedAccepter(rw))[1] is rw
    unknown = object()
    layers, found = _unwrap_accepter(ConstrainAccepter(unknown, below))  # returned, not raised
    assert len(layers) == 1 and found is unknown


def test_device_plan_objections():
    with pytest.raises(UnsupportedOnDevice, match="needs a BoxConstraint"):
        _Plan(PROPOSER, CountedAccepter(ConstrainAccepter(pCNAccepter(_phi), below)))
    box = BoxConstraint(-1, 1)
    with pytest.raises(UnsupportedOnDevice, match="only one ConstrainAccepter"):
        _Plan(PROPOSER, ConstrainAccepter(CountedAccepter(ConstrainAccepter(pCNAccepter(_phi), box)), box))
    with pytest.raises(UnsupportedOnDevice, match="needs a pCNAccepter or StandardRWAccepter, not object"):
        _Plan(PROPOSER, CountedAccepter(object()))
    # outermost first: the second ConstrainAccepter is met before its predicate or the core beneath it
    with pytest.raises(UnsupportedOnDevice, match="only one ConstrainAccepter"):
        _Plan(PROPOSER, ConstrainAccepter(ConstrainAccepter(object(), below), box))
    with pytest.raises(UnsupportedOnDevice, match="needs a BoxConstraint"):
        _Plan(PROPOSER, ConstrainAccepter(ConstrainAccepter(object(), box), below))
    with pytest.raises(UnsupportedOnDevice, match="must be an EvolutionPotential"):
        _Plan(PROPOSER, CountedAccepter(ConstrainAccepter(CountedAccepter(pCNAccepter(_phi)), box)))


def test_host_plan_objections():
    box = BoxConstraint(-1, 1)
    inner = CountedAccepter(pCNAccepter(_phi))
    outer = CountedAccepter(ConstrainAccepter(ConstrainAccepter(inner, below), box))
    plan = HostPlan(PROPOSER, outer, 2)  # any predicate, any number of them
    assert [kind for kind, _ in plan.layers] == ["count", "constrain", "constrain", "count"]
    assert plan.layers[0][1] is outer and plan.layers[1][1] is box and plan.layers[2][1] is below
    assert plan.layers[3][1] is inner and plan.reg_prior is None and plan.accept_kind == "pcn"
    rw = HostPlan(PROPOSER, StandardRWAccepter(_phi, PRIOR), 2)
    assert rw.layers == [] and rw.reg_prior is PRIOR and rw.accept_kind == "rw_reg"
    with pytest.raises(GenericComposition, match="object"):
        HostPlan(PROPOSER, CountedAccepter(ConstrainAccepter(object(), below)), 2)


def test_tempered_smc_objections():
    with pytest.raises(NotImplementedError, match="ConstrainAccepter is not supported"):
        TemperedSMC(PRIOR, CountedAccepter(ConstrainAccepter(StandardRWAccepter(_phi, PRIOR), below)))
    with pytest.raises(NotImplementedError, match="random-walk accepters"):
        TemperedSMC(PRIOR, CountedAccepter(StandardRWAccepter(_phi, PRIOR)))
    with pytest.raises(TypeError, match="must be an EvolutionPotential, not function"):
        TemperedSMC(PRIOR, CountedAccepter(pCNAccepter(_phi)))
