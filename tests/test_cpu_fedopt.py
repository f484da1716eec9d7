"""CPU: FedAdagrad and FedYogi in the server step, everything that needs no device.

  * validation and parsing: Optim, main.parse, FLSimulation and the C entry points refuse the
    hyper-parameters torch's constructors refuse (status 1, a message that is no null-pointer
    message, before any pointer check or launch);
  * the yardsticks of tests/test_gpu_fedopt.py (tests/_fedopt.py) against the real thing:
    adagrad_expected against torch.optim.Adagrad.step() itself, and flsim.optim.Yogi (the rule
    text as an optimizer class) against yogi_expected.

The yardsticks take a correctly rounded sqrt (numpy's) where torch takes its vectorised one, which
is within 1 ulp.  So the state arrays, which no sqrt enters, must have zero differing words, and p
may differ only where torch's root differs from the correctly rounded one, on at most 0.5 % of the
elements (the project's cap for Adam against torch's sqrt), each by at most 2^-21 |update| +
2^-23 |p|: a denominator 1 ulp off (2^-23 relative, eps only shrinks it), two roundings of the
quotient and one of p give half of that.

Measured: where torch's sqrt differs from the correctly rounded one on 0.6 - 0.9 % of the values
(the premise of the 0.5 % cap), p differs on 0 - 0.058 % of the elements and
reaches 0.93 of the bound.  Which sqrt torch runs depends on the CPU its maths library dispatches
for.  On one where 7 - 18 % of the roots are 1 ulp off, every differing element of p still sits at a
differing root and stays within the bound (0.98 of it at the most), but the 0.5 % cap is missed
in three cases: adagrad "all" step 1 at 0.639 %, yogi "betas" at 1.072 % (P = 305,141) and 1.094 %
(P = 5,212); the others reach 0.013 - 0.499 %.  The cap stands as the project set it: on such a
CPU those three cases fail.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

import _fedopt as F

P_BIG, P_SMALL = 305_141, 5_212
NAN = float("nan")

# ---- validation and parsing --------------------------------------------------------------------


def test_optim_kinds_validate_and_carry_their_fields():
    from flsim._lib import OPT_KINDS
    from flsim.engine import Optim, optim_defaults
    assert (OPT_KINDS["adagrad"], OPT_KINDS["yogi"]) == (3, 4)
    a = Optim(kind="adagrad", lr=0.01, lr_decay=0.5, eps=1e-10, weight_decay=1e-3,
              initial_accumulator_value=0.1).validate()
    y = Optim(kind="yogi", lr=0.01, betas=(0.8, 0.95), eps=1e-3,
              initial_accumulator_value=1e-6).validate()
    assert (a.n_state, y.n_state) == (1, 2)
    ca, cy = a.c_struct(), y.c_struct()
    assert (ca.kind, ca.lr, ca.lr_decay, ca.eps, ca.weight_decay) == (3, 0.01, 0.5, 1e-10, 1e-3)
    assert (cy.kind, cy.beta1, cy.beta2, cy.eps, cy.lr_decay) == (4, 0.8, 0.95, 1e-3, 0.0)
    # the other kinds are as they were
    assert Optim().lr_decay == 0.0 and Optim().initial_accumulator_value == 0.0
    assert (Optim(kind="sgd", momentum=0.9).n_state, Optim(kind="adamw").n_state) == (1, 2)
    assert optim_defaults("adagrad") == dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-10,
                                             initial_accumulator_value=0.0)
    assert optim_defaults("yogi") == dict(lr=1e-2, betas=(0.9, 0.99), eps=1e-3,
                                          initial_accumulator_value=1e-6)
    assert optim_defaults("adam") == dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                                          initial_accumulator_value=0.0)
    with pytest.raises(ValueError):
        optim_defaults("rmsprop")


@pytest.mark.parametrize("kw,match", [
    (dict(kind="adagrad", lr_decay=-1.0), "lr_decay"),
    (dict(kind="adagrad", lr_decay=NAN), "lr_decay"),
    (dict(kind="adagrad", eps=-1e-10), "epsilon"),
    (dict(kind="adagrad", initial_accumulator_value=-0.1), "initial_accumulator_value"),
    (dict(kind="adagrad", lr=-0.1), "learning rate"),
    (dict(kind="adagrad", weight_decay=-0.1), "weight_decay"),
    (dict(kind="yogi", eps=-1e-3), "epsilon"),
    (dict(kind="yogi", eps=NAN), "epsilon"),
    (dict(kind="yogi", betas=(1.0, 0.99)), "index 0"),
    (dict(kind="yogi", betas=(-0.1, 0.99)), "index 0"),
    (dict(kind="yogi", betas=(0.9, 1.0)), "index 1"),
    (dict(kind="yogi", betas=(0.9, NAN)), "index 1"),
    (dict(kind="yogi", initial_accumulator_value=-1e-6), "initial_accumulator_value"),
    (dict(kind="rmsprop"), "rmsprop"),
])
def test_python_optim_refuses_what_torch_refuses(kw, match):
    from flsim.engine import Optim
    with pytest.raises(ValueError, match=match):
        Optim(**kw).validate()


def test_torch_adagrad_refuses_the_same_cases():
    """The messages Optim.validate() matches are torch's own."""
    p = [torch.nn.Parameter(torch.zeros(3))]
    for kw, match in ((dict(lr_decay=-1.0), "lr_decay"), (dict(eps=-1e-10), "epsilon"),
                      (dict(initial_accumulator_value=-0.1), "initial_accumulator_value"),
                      (dict(weight_decay=-0.1), "weight_decay"), (dict(lr=-0.1), "learning rate")):
        with pytest.raises(ValueError, match=match):
            torch.optim.Adagrad(p, **kw)
    from flsim.optim import Yogi
    for kw, match in ((dict(eps=-1e-3), "epsilon"), (dict(betas=(1.0, 0.99)), "index 0"),
                      (dict(betas=(0.9, 1.0)), "index 1"), (dict(lr=-1.0), "learning rate"),
                      (dict(initial_accumulator_value=-1.0), "initial_accumulator_value"),
                      (dict(weight_decay=-1.0), "weight_decay")):
        with pytest.raises(ValueError, match=match):
            Yogi(p, **kw)


def test_main_parses_the_new_flags():
    import main
    a = main.parse([])
    assert (a.optimizer, a.lr_decay, a.initial_accumulator_value, a.eps, a.beta1, a.beta2) == \
        ("adam", 0.0, None, None, None, None)
    assert main.optim_kwargs(a) == dict(lr_decay=0.0, initial_accumulator_value=None, eps=None,
                                        betas=(0.9, 0.999))
    a = main.parse(["--optimizer", "yogi", "--learning_rate", "0.01", "--beta2", "0.95", "--eps",
                    "1e-2", "--initial_accumulator_value", "1e-4", "--weight_decay", "1e-3"])
    assert (a.optimizer, a.beta1, a.beta2, a.eps, a.initial_accumulator_value) == \
        ("yogi", None, 0.95, 1e-2, 1e-4)
    assert main.optim_kwargs(a)["betas"] == (0.9, 0.95)
    assert main.optim_kwargs(main.parse(["--optimizer", "yogi"]))["betas"] == (0.9, 0.99)
    a = main.parse(["--optimizer", "adagrad", "--lr_decay", "0.1", "--beta1", "0.5"])
    assert (a.optimizer, a.lr_decay) == ("adagrad", 0.1)
    assert main.optim_kwargs(a)["betas"] == (0.5, 0.999)
    with pytest.raises(SystemExit):
        main.parse(["--optimizer", "rmsprop"])


@pytest.mark.parametrize("kw,match", [
    (dict(optimizer="adagrad", lr_decay=-1), "lr_decay"),
    (dict(optimizer="adagrad", initial_accumulator_value=-1.0), "initial_accumulator_value"),
    (dict(optimizer="adagrad", eps=-1.0), "epsilon"),
    (dict(optimizer="yogi", betas=(0.9, 1.0)), "index 1"),
    (dict(optimizer="rmsprop"), "rmsprop"),
])
def test_simulation_refuses_before_any_device_use(kw, match):
    from flsim.sim import FLSimulation
    with pytest.raises(ValueError, match=match):
        FLSimulation(4, delay=2, **kw)


BAD = {
    "unknown_kind": (dict(kind=7), "unknown optimizer kind 7"),
    "adagrad_lr_decay": (dict(kind=3, lr_decay=-0.5), "Invalid lr_decay value"),
    "adagrad_lr_decay_nan": (dict(kind=3, lr_decay=NAN), "Invalid lr_decay value"),
    "adagrad_eps": (dict(kind=3, eps=-1e-10), "Invalid epsilon value"),
    "adagrad_eps_nan": (dict(kind=3, eps=NAN), "Invalid epsilon value"),
    "adagrad_lr": (dict(kind=3, lr=-0.1), "Invalid learning rate"),
    "adagrad_weight_decay": (dict(kind=3, weight_decay=-0.1), "Invalid weight_decay value"),
    "yogi_eps": (dict(kind=4, eps=-1e-3), "Invalid epsilon value"),
    "yogi_eps_nan": (dict(kind=4, eps=NAN), "Invalid epsilon value"),
    "yogi_beta1_one": (dict(kind=4, beta1=1.0), "Invalid beta parameter at index 0"),
    "yogi_beta1_negative": (dict(kind=4, beta1=-0.1), "Invalid beta parameter at index 0"),
    "yogi_beta1_nan": (dict(kind=4, beta1=NAN), "Invalid beta parameter at index 0"),
    "yogi_beta2_one": (dict(kind=4, beta2=1.0), "Invalid beta parameter at index 1"),
    "yogi_beta2_nan": (dict(kind=4, beta2=NAN), "Invalid beta parameter at index 1"),
    "yogi_lr_nan": (dict(kind=4, lr=NAN), "Invalid learning rate"),
}


def _c_optim(**kw):
    from flsim._lib import FlsimOptim
    o = FlsimOptim()
    o.kind, o.nesterov = 0, 0
    o.lr, o.beta1, o.beta2, o.eps = 1e-2, 0.9, 0.99, 1e-3
    o.weight_decay = o.momentum = o.dampening = o.lr_decay = 0.0
    for k, v in kw.items():
        setattr(o, k, v)
    return o


@pytest.mark.parametrize("case", sorted(BAD))
def test_entry_points_refuse_before_any_pointer_check(case):
    from flsim._lib import lib
    L = lib()
    kw, text = BAD[case]
    o = ctypes.byref(_c_optim(**kw))
    N = None
    calls = [
        lambda: L.flsim_aggregate_optim_rule_push(N, N, N, N, N, N, 0, N, 0, 1, o, N),
        lambda: L.flsim_aggregate_optim_wrule_push(N, N, N, N, N, N, N, 0, N, 0, 1, o, N),
        lambda: L.flsim_aggregate_optim_crule_push(N, N, N, N, N, N, N, N, N, 0, N, 0, 1, o, N),
        lambda: L.flsim_aggregate_optim_clip_push(N, N, N, N, N, N, N, N, N, N, 0, N, 0, 1, o, N),
    ]
    for net in ("pn1", "vgg11", "vgg11_bn"):
        f = getattr(L, f"flsim_{net}_server_step_optim")
        calls.append(lambda f=f: f(N, N, N, N, N, N, 1, o, N))
        f = getattr(L, f"flsim_{net}_server_step_wrule")
        calls.append(lambda f=f: f(N, N, N, N, N, N, N, 1, o, N))
        f = getattr(L, f"flsim_{net}_server_step_crule")
        calls.append(lambda f=f: f(N, N, N, N, N, N, N, N, N, 1, o, N))
    for call in calls:
        assert call() == 1
        msg = L.flsim_last_error().decode()
        assert text in msg and "null pointer" not in msg, msg


def test_valid_new_kinds_reach_the_pointer_check():
    """A valid Adagrad / Yogi gets past the hyper-parameter checks: the refusal is then the
    null-pointer one (nothing is launched).  lr_decay is read for Adagrad only."""
    from flsim._lib import lib
    L = lib()
    for kw in (dict(kind=3, lr_decay=0.1, eps=1e-10), dict(kind=4), dict(kind=4, lr_decay=-1.0),
               dict(kind=0, lr_decay=NAN), dict(kind=4, beta1=0.0, beta2=0.0, eps=0.0)):
        o = ctypes.byref(_c_optim(**kw))
        assert L.flsim_aggregate_optim_rule_push(None, None, None, None, None, None, 0, None, 0, 1,
                                                 o, None) == 1
        assert "null pointer" in L.flsim_last_error().decode(), kw


# ---- the yardsticks ----------------------------------------------------------------------------
def _gradient(rs, n):
    """+-0 and a subnormal among ordinary values."""
    g = (rs.standard_normal(n) * 1e-2).astype(np.float32)
    g[::17] = 0.0
    g[1::17] = -0.0
    g[2::17] = np.float32(3e-39) * rs.choice([-1, 1], len(g[2::17]))
    return g


ADAGRAD_SETTINGS = {
    "plain": dict(),
    "decay_wd": dict(lr_decay=0.05, weight_decay=5e-4),
    "accumulator": dict(initial_accumulator_value=0.1),
    "all": dict(lr=0.05, lr_decay=0.05, weight_decay=5e-4, initial_accumulator_value=1e-3,
                eps=1e-8),
}


@pytest.mark.parametrize("step", [1, 3])
@pytest.mark.parametrize("setting", sorted(ADAGRAD_SETTINGS))
def test_adagrad_helper_against_torch_adagrad_step(setting, step):
    hp = ADAGRAD_SETTINGS[setting]
    rs = np.random.RandomState(100 * step + sorted(ADAGRAD_SETTINGS).index(setting))
    g, p = _gradient(rs, P_BIG), rs.standard_normal(P_BIG).astype(np.float32)
    iav = hp.get("initial_accumulator_value", 0.0)
    # step 1: the sum torch's constructor fills; step 3: what two steps would have left
    s0 = np.full(P_BIG, iav, np.float32)
    if step > 1:
        s0 = (s0 + (rs.rand(P_BIG) * 2e-4).astype(np.float32)).astype(np.float32)
    tp = torch.nn.Parameter(torch.from_numpy(p.copy()))
    opt = torch.optim.Adagrad([tp], **hp)
    assert F.n_diff(opt.state[tp]["sum"], np.full(P_BIG, iav, np.float32)) == 0
    if step > 1:
        opt.state[tp]["sum"] = torch.from_numpy(s0.copy())
        opt.state[tp]["step"] = torch.tensor(float(step - 1))
    tp.grad = torch.from_numpy(g.copy())
    opt.step()
    assert float(opt.state[tp]["step"]) == step
    ref = {k: v for k, v in hp.items() if k != "initial_accumulator_value"}
    pe, se = F.adagrad_expected(g, p, s0, step, **ref)
    assert F.n_diff(opt.state[tp]["sum"], se) == 0
    F.check_sqrt_close(tp.detach().numpy(), pe, p, se, f"adagrad {setting} step {step}")
    # with torch's own sqrt in the helper: the same ops, zero differing words
    pt, st = F.adagrad_expected(g, p, s0, step, sqrt=torch.sqrt, **ref)
    assert F.n_diff(tp, pt) == 0 and F.n_diff(opt.state[tp]["sum"], st) == 0
    assert F.n_diff(pe, p) > P_BIG // 2          # the step acts


def _yogi_gradient(rs, n):
    g = _gradient(rs, n)
    g[3::17] = np.float32(1e30)                  # g * g = inf
    return g


YOGI_SETTINGS = {
    "plain": dict(),
    "wd": dict(weight_decay=5e-4),
    "betas": dict(lr=0.05, betas=(0.5, 0.9), eps=1e-5, weight_decay=1e-3),
    "beta1_zero": dict(betas=(0.0, 0.99)),
}


def _yogi_state(opt, tp, m, v, step):
    opt.state[tp] = {"step": torch.tensor(float(step)), "exp_avg": torch.from_numpy(m.copy()),
                     "exp_avg_sq": torch.from_numpy(v.copy())}


@pytest.mark.parametrize("P", [P_BIG, P_SMALL])
@pytest.mark.parametrize("setting", sorted(YOGI_SETTINGS))
def test_yogi_class_against_yogi_expected(setting, P):
    """One step from a random state (all three signs of v - g^2, and g^2 = inf) and three steps
    from the initial state."""
    from flsim.optim import Yogi
    hp = YOGI_SETTINGS[setting]
    rs = np.random.RandomState(P % 1000 + sorted(YOGI_SETTINGS).index(setting))
    g, p = _yogi_gradient(rs, P), rs.standard_normal(P).astype(np.float32)
    m = (rs.standard_normal(P) * 1e-3).astype(np.float32)
    v = (rs.rand(P) * 2e-4).astype(np.float32)
    with np.errstate(over="ignore"):
        g2 = g * g
    if not hp.get("weight_decay"):
        v[5::17] = g2[5::17]                     # sign 0
    for sqrt in (None, F.sqrt_rn):
        tp = torch.nn.Parameter(torch.from_numpy(p.copy()))
        opt = Yogi([tp], **hp)
        if sqrt is not None:
            opt._sqrt = sqrt                     # the class with numpy's sqrt substituted
        _yogi_state(opt, tp, m, v, 2)
        tp.grad = torch.from_numpy(g.copy())
        opt.step()
        pe, me, ve = F.yogi_expected(g, p, m, v, 3, **hp)
        st = opt.state[tp]
        assert float(st["step"]) == 3
        assert F.n_diff(st["exp_avg"], me) == 0 and F.n_diff(st["exp_avg_sq"], ve) == 0
        if sqrt is not None:
            assert F.n_diff(tp, pe) == 0
        else:
            F.check_sqrt_close(tp.detach().numpy(), pe, p, ve, f"yogi {setting} P {P}")
    if not hp.get("weight_decay"):
        d = v - g2
        shares = [float((d > 0).mean()), float((d == 0).mean()), float((d < 0).mean())]
        assert min(shares) > 0.05, shares
    assert np.isinf(ve[3::17]).all()             # g^2 = inf lands in v
    # three steps from the initial state, numpy's sqrt in the class: bit for bit throughout
    iav = 1e-6
    tp = torch.nn.Parameter(torch.from_numpy(p.copy()))
    opt = Yogi([tp], initial_accumulator_value=iav, **hp)
    opt._sqrt = F.sqrt_rn
    pe, me, ve = p.copy(), np.zeros(P, np.float32), np.full(P, iav, np.float32)
    for step in (1, 2, 3):
        gs = _yogi_gradient(rs, P)
        tp.grad = torch.from_numpy(gs.copy())
        opt.step()
        pe, me, ve = F.yogi_expected(gs, pe, me, ve, step, **hp)
        st = opt.state[tp]
        assert (F.n_diff(tp, pe), F.n_diff(st["exp_avg"], me), F.n_diff(st["exp_avg_sq"], ve)) == \
            (0, 0, 0), step
    # the second g^2 = inf on v = inf: sign(NaN) = 0 and -+0 * inf is NaN, as torch has it
    assert np.isnan(ve[3::17]).all() and np.isfinite(ve[4::17]).all()


def test_yogi_state_dict_round_trip():
    from flsim.optim import Yogi
    tp = torch.nn.Parameter(torch.ones(5))
    opt = Yogi([tp], initial_accumulator_value=0.25)
    tp.grad = torch.full((5,), 2.0)
    opt.step()
    st = opt.state[tp]
    assert sorted(st) == ["exp_avg", "exp_avg_sq", "step"]
    # v = 0.25 - 0.01 * sign(0.25 - 4) * 4 = 0.29; m = 0.2
    assert torch.allclose(st["exp_avg_sq"], torch.full((5,), 0.29))
    assert torch.allclose(st["exp_avg"], torch.full((5,), 0.2))
    assert torch.allclose(tp, torch.full((5,), 1 - 1e-2 * 0.2 / (math.sqrt(0.29) + 1e-3)))
    fresh = Yogi([torch.nn.Parameter(torch.ones(5))])
    fresh.load_state_dict(opt.state_dict())
    assert fresh.param_groups[0]["initial_accumulator_value"] == 0.25
