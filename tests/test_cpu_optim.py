"""CPU: the optimizer-taking entry points refuse the hyper-parameters torch's constructors refuse
(status 1 and a message, before any pointer check or launch), and the command line carries the
optimizer flags.  Only invalid inputs are passed, so nothing is launched.
"""
import ctypes

import pytest

BAD = {
    "unknown_kind": dict(kind=7),
    "negative_lr": dict(kind=2, lr=-0.1),
    "negative_lr_adam": dict(kind=0, lr=-1e-3),
    "negative_weight_decay": dict(kind=1, weight_decay=-1e-2),
    "negative_weight_decay_sgd": dict(kind=2, weight_decay=-5e-4),
    "negative_momentum": dict(kind=2, momentum=-0.9),
    "nesterov_without_momentum": dict(kind=2, nesterov=1, momentum=0.0),
    "nesterov_with_dampening": dict(kind=2, nesterov=1, momentum=0.9, dampening=0.1),
    "nesterov_negative_momentum": dict(kind=2, nesterov=1, momentum=-0.5),
}


def _optim(**kw):
    from flsim._lib import FlsimOptim
    o = FlsimOptim()
    o.kind, o.nesterov = 0, 0
    o.lr, o.beta1, o.beta2, o.eps = 1e-3, 0.9, 0.999, 1e-8
    o.weight_decay = o.momentum = o.dampening = 0.0
    for k, v in kw.items():
        setattr(o, k, v)
    return o


@pytest.mark.parametrize("case", sorted(BAD))
def test_invalid_hyper_parameters_are_refused(case):
    from flsim._lib import lib
    L = lib()
    o = _optim(**BAD[case])
    calls = [lambda: L.flsim_aggregate_optim_rule_push(None, None, None, None, None, None, 0, None,
                                                       0, 1, ctypes.byref(o), None)]
    for net in ("pn1", "vgg11", "vgg11_bn"):
        fn = getattr(L, f"flsim_{net}_server_step_optim")
        calls.append(lambda fn=fn: fn(None, None, None, None, None, None, 1, ctypes.byref(o),
                                      None))
    for call in calls:
        assert call() == 1
        msg = L.flsim_last_error().decode()
        assert msg and "null pointer" not in msg, msg


def test_python_optim_refuses_the_same_cases():
    from flsim.engine import Optim
    for kw in (dict(kind="rmsprop"), dict(kind="sgd", lr=-0.1), dict(kind="adamw", weight_decay=-1),
               dict(kind="sgd", momentum=-0.9), dict(kind="sgd", nesterov=True),
               dict(kind="sgd", nesterov=True, momentum=0.9, dampening=0.1)):
        with pytest.raises(ValueError):
            Optim(**kw).validate()
    o = Optim(kind="sgd", momentum=0.9, nesterov=True).validate()
    assert (o.n_state, Optim(kind="sgd").n_state, Optim(kind="adamw").n_state) == (1, 0, 2)
    c = o.c_struct()
    assert (c.kind, c.nesterov, c.momentum) == (2, 1, 0.9)


def test_main_parses_the_optimizer_flags():
    import main
    a = main.parse([])
    assert (a.optimizer, a.momentum, a.dampening, a.nesterov, a.weight_decay) == \
        ("adam", 0.0, 0.0, False, 0.0)
    a = main.parse(["--optimizer", "sgd", "--momentum", "0.9", "--dampening", "0.1",
                    "--weight_decay", "5e-4", "--learning_rate", "0.01"])
    assert (a.optimizer, a.momentum, a.dampening, a.nesterov, a.weight_decay, a.learning_rate) == \
        ("sgd", 0.9, 0.1, False, 5e-4, 0.01)
    assert main.parse(["--optimizer", "sgd", "--momentum", "0.9", "--nesterov"]).nesterov is True
    with pytest.raises(SystemExit):
        main.parse(["--optimizer", "rmsprop"])


def test_nesterov_without_momentum_fails_before_any_device_use():
    import main
    for argv in (["--nesterov"], ["--optimizer", "sgd", "--nesterov"]):
        a = main.parse(argv)
        _construct_raises(a)


def _construct_raises(a):
    from flsim.sim import FLSimulation
    with pytest.raises(ValueError, match="[Nn]esterov"):
        FLSimulation(a.n_workers, delay=a.delay, lr=a.learning_rate, optimizer=a.optimizer,
                     weight_decay=a.weight_decay, momentum=a.momentum, dampening=a.dampening,
                     nesterov=a.nesterov)
