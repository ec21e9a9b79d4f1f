"""Host: the solvers' hyperparameters are the two descriptors of solvers/hyper.py, each objective's hook is one class shared
by its VAE and Soft-Intro solvers, and the VAE step, its tail and the parameter-group methods exist once.  Solvers are
built on the CPU (nothing here runs a kernel) at zdim=10, channels=(8, 16), image_size=16."""
import math

import pytest
import torch

NET = dict(cdim=3, zdim=10, channels=(8, 16), image_size=16)
ALL = ("VAESolver", "IntroSolver", "TCSovler", "IntroTCSovler", "DIPSolver", "IntroDIPSolver", "MMDSolver",
       "IntroMMDSolver", "FactorSolver", "AdaGVAESolver", "JointVAESolver", "AnnealedVAESolver")
# class -> the hyperparameters it declares
DECLARED = {
    "VAESolver": (), "IntroSolver": (),
    "TCSovler": ("kl_loss",), "IntroTCSovler": ("kl_loss",),
    "DIPSolver": ("dip_type", "lambda_od", "lambda_d"), "IntroDIPSolver": ("dip_type", "lambda_od", "lambda_d"),
    "MMDSolver": ("lambda_mmd", "mmd_kernel", "mmd_bandwidth"),
    "IntroMMDSolver": ("lambda_mmd", "mmd_kernel", "mmd_bandwidth"),
    "FactorSolver": ("gamma",), "AdaGVAESolver": ("averaging",),
    "JointVAESolver": ("temperature", "gamma_cont", "gamma_disc"),
    "AnnealedVAESolver": ("temperature", "gamma_cont", "gamma_disc"),
}
PAIRS = (("TCSovler", "IntroTCSovler"), ("DIPSolver", "IntroDIPSolver"), ("MMDSolver", "IntroMMDSolver"))


def _cls(name):
    import solvers
    return getattr(solvers, name)


def _solver(name, **kw):
    import models
    cls = _cls(name)
    m = models.SoftIntroVAE(arch="conv", **NET)

    class DS:
        def __len__(self):
            return 100

    args = [DS(), m, 4, torch.optim.Adam(m.encoder.parameters()), torch.optim.Adam(m.decoder.parameters()), "mse",
            0.5, 0.75]
    if name.startswith("Intro"):
        args += [512.0, 1e-8]
    if name == "FactorSolver":
        disc = models.Discriminator(NET["zdim"], hidden=16, layers=2)
        kw.update(discriminator=disc, optimizer_disc=torch.optim.Adam(disc.parameters(), lr=1e-4, betas=(0.5, 0.9)))
    return cls(*args, torch.device("cpu"), False, None, **kw)


def _descriptors(cls):
    from solvers.hyper import Choice, Number
    return {n: d for k in reversed(cls.__mro__) for n, d in vars(k).items() if isinstance(d, (Choice, Number))}


def _key(s):
    """What the hyperparameters reach of the captured graph's key: the solver's extension and the KL mode that
    ``_run_scoped`` puts at the key's end."""
    return s._graph_key_extra() + (getattr(s, "kl_loss", None),)


CASES = [(c, n) for c in ALL for n in DECLARED[c]]


def test_every_class_declares_its_hyperparameters_and_nothing_else():
    for name in ALL:
        assert tuple(_descriptors(_cls(name))) == DECLARED[name], name


@pytest.mark.parametrize("name,attr", CASES, ids=[f"{c}-{n}" for c, n in CASES])
def test_descriptor_checks_every_assignment(name, attr):
    from solvers.hyper import Choice
    cls = _cls(name)
    d = _descriptors(cls)[attr]
    assert getattr(cls, attr) is d and d.name == attr                   # class-level access: the descriptor itself
    s = _solver(name)
    slot = "_" + attr
    if isinstance(d, Choice):
        bad = ["nope", d.options[0].upper(), "", None, 1, True]
        good = [o for o in d.options if o != getattr(s, attr)]
    else:
        bad = [-1.0, -1, float("nan"), float("inf"), float("-inf"), "3", True, False, 1 + 0j, [1.0]]
        bad += [0, 0.0] if d.positive else []
        bad += [] if d.optional else [None]
        good = [3, 1.5]                                                   # an int is stored as a float
    for value in bad:
        before = s.__dict__[slot]
        with pytest.raises(ValueError, match=attr):
            setattr(s, attr, value)
        assert s.__dict__[slot] is before, (attr, value)
    for value in good:
        key = _key(s)
        setattr(s, attr, value)
        got = s.__dict__[slot]
        assert got == value and type(got) is (str if isinstance(d, Choice) else float)
        assert getattr(s, attr) == got
        assert _key(s) != key, (attr, value)
    if not isinstance(d, Choice):
        if not d.positive:
            setattr(s, attr, 0)
            assert s.__dict__[slot] == 0.0
        if d.optional:
            setattr(s, attr, None)
            assert s.__dict__[slot] is None


@pytest.mark.parametrize("name", ["DIPSolver", "IntroDIPSolver"])
def test_lambda_d_fallback_follows_kind_and_lambda_od_at_every_read(name):
    s = _solver(name)
    assert s.__dict__["_lambda_d"] is None and s.lambda_d == 100.0
    for kind, od in (("ii", 4), ("i", 4), ("i", 0.5), ("ii", 0.5), ("ii", 0)):
        s.dip_type, s.lambda_od = kind, od
        assert s.lambda_d == (10.0 if kind == "i" else 1.0) * od and s.__dict__["_lambda_d"] is None
        assert s._graph_key_extra()[-3:] == (kind, float(od), s.lambda_d)
    s.lambda_d = 2.5
    s.dip_type, s.lambda_od = "i", 7.0
    assert s.lambda_d == 2.5
    s.lambda_d = None
    assert s.lambda_d == 70.0


def test_joint_numbers_are_strict_like_the_rest():
    """The one narrowing: ``float()`` used to coerce strings and bools for these three."""
    for attr in ("temperature", "gamma_cont", "gamma_disc"):
        s = _solver("JointVAESolver")
        for value in ("3", True, None, "x"):
            with pytest.raises(ValueError, match=attr):
                setattr(s, attr, value)
    s = _solver("AnnealedVAESolver", gamma=7)
    assert s.gamma == s.gamma_cont == 7.0
    s.gamma = 9
    assert s.gamma_cont == 9.0 and math.isclose(s.temperature, 0.67)


def test_twins_share_their_hook():
    """A Soft-Intro solver and its VAE sibling resolve the hook to the same function objects, and neither has a body of its
    own.  The TC hook has no graph-key extension (``_run_scoped`` ends every key with ``kl_loss``), so for that pair
    ``_graph_key_extra`` stays the step class's."""
    from solvers import IntroSolver, VAESolver
    for vae, intro in PAIRS:
        a, b = _cls(vae), _cls(intro)
        assert set(vars(a)) <= {"__module__", "__doc__"} and set(vars(b)) <= {"__module__", "__doc__"}, (vae, intro)
        assert issubclass(a, VAESolver) and not issubclass(a, IntroSolver) and issubclass(b, IntroSolver)
        assert a.compute_kl_loss is b.compute_kl_loss and a.compute_kl_loss is not VAESolver.compute_kl_loss
        assert a.__init__ is b.__init__
        if vae == "TCSovler":
            for n in ("_compute_kl_loss_simple", "_compute_kl_loss_full", "kl_decomposition"):
                assert getattr(a, n) is getattr(b, n)
            assert a._graph_key_extra is VAESolver._graph_key_extra and b._graph_key_extra is IntroSolver._graph_key_extra
        else:
            assert a._graph_key_extra is b._graph_key_extra
            assert a._graph_key_extra is not VAESolver._graph_key_extra


def test_the_step_and_the_group_methods_exist_once():
    from solvers import IntroSolver, VAESolver
    for n in ("_params", "_group", "_step"):
        assert n not in vars(_cls("FactorSolver")), n
        assert all(n not in vars(_cls(c)) for c in ALL if c != "VAESolver"), n
    for c in ("AdaGVAESolver", "JointVAESolver", "AnnealedVAESolver", "FactorSolver"):
        assert "_device_step" not in vars(_cls(c)) and "train_step" not in vars(_cls(c)), c
        assert _cls(c)._device_step is VAESolver._device_step and _cls(c).train_step is VAESolver.train_step
    assert "_device_step" in vars(IntroSolver) and "train_step" in vars(IntroSolver)
    # the third group goes through the two lookups
    s = _solver("FactorSolver")
    assert s._module("discriminator") is s.discriminator and s._optimizer("discriminator") is s.optimizer_disc
    assert s._module("encoder") is s.model.encoder and s._optimizer("encoder") is s.optimizer_e
    assert s._optimizer("decoder") is s.optimizer_d
    assert [id(p) for p in s._params("discriminator")] == [id(p) for p in s.discriminator.parameters()]
    assert s._updates == ("encoder", "decoder", "discriminator") and VAESolver._updates == ("encoder", "decoder")


def test_package_exports_the_twelve():
    import solvers
    assert sorted(solvers.__all__) == sorted(ALL)
    for name in ALL:
        assert getattr(solvers, name).__name__ == name
    from solvers.ada import ADA_AVERAGINGS
    from solvers.dip import DIP_TYPES
    from solvers.mmd import MMD_KERNELS
    from solvers.tc import KL_LOSSES
    assert (DIP_TYPES, MMD_KERNELS, KL_LOSSES) == (("i", "ii"), ("imq", "rbf"), ("simple", "full"))
    assert set(ADA_AVERAGINGS) == {"gvae", "mlvae"}
