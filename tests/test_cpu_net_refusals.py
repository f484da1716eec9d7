"""CPU: the network entry points (flsim_pn1_*, flsim_vgg11_*, flsim_vgg11_bn_*) refuse bad
arguments with status 1 and a fixed message, before anything is launched.  Every pointer is a
fake non-null host address and each call carries one invalid argument, so only refused calls are
made.  engine.py's check() turns the status and message into the exception the caller sees, so
the texts are part of the behaviour.
"""
import ctypes

import pytest

NETS = ("pn1", "vgg11", "vgg11_bn")
P = ctypes.c_void_p(0x1000)          # never dereferenced: every call is refused first
ST = ctypes.c_void_p(0)              # the null stream
SEED = ctypes.c_uint64(1)


def _refused(rc, text):
    from flsim._lib import lib
    assert rc == 1
    assert lib().flsim_last_error().decode() == text


def _fn(net, name):
    from flsim._lib import lib
    return getattr(lib(), f"flsim_{net}_{name}")


def _bn(net):
    return (P,) if net == "vgg11_bn" else ()


def chunk(net, max_samples=256, len_a=4, n_chunk=1, workspace=P):
    return _fn(net, "fwd_bwd_chunk")(P, workspace, max_samples, P, P, P, P, len_a, P, 4, P, P,
                                     n_chunk, 8, SEED, 1, 1, P, *_bn(net), ST)


def batch(net, n_samples, max_samples=256):
    return _fn(net, "fwd_bwd_input")(P, P, max_samples, P, P, P, n_samples, P, SEED, 1, 1, P,
                                     *_bn(net), ST)


def load_rows(net, max_samples, row0, n_samples):
    return _fn(net, "load_rows")(P, P, max_samples, row0, P, P, n_samples, ST)


@pytest.mark.parametrize("net", NETS)
def test_chunk_refusals(net):
    _refused(chunk(net, n_chunk=0), "empty chunk")
    _refused(chunk(net, max_samples=128, n_chunk=2),
             "chunk of 256 samples exceeds workspace (128)")
    _refused(chunk(net, max_samples=32768, n_chunk=129),
             "chunk of 16512 samples exceeds the 32-bit index budget")
    _refused(chunk(net, len_a=0), "empty class list")
    _refused(chunk(net, workspace=None), "null pointer")


@pytest.mark.parametrize("net", NETS)
def test_batch_refusals(net):
    _refused(batch(net, 0), "empty batch")
    # vgg11_bn: one BatchNorm batch per 128-sample group, so ragged batches are refused first
    _refused(batch(net, 200, max_samples=128),
             "vgg11_bn batch of 200 samples: must be a multiple of 128" if net == "vgg11_bn"
             else "batch of 200 samples exceeds workspace (128)")


@pytest.mark.parametrize("net", NETS)
def test_load_rows_refusals(net):
    _refused(load_rows(net, 256, 64, 128), "row0 64 is not a multiple of 128")
    _refused(load_rows(net, 256, 128, 256), "rows [128, 384) exceed workspace (256)")
    _refused(load_rows(net, 32768, 0, 128),
             "workspace of 32768 samples exceeds the 32-bit index budget")


@pytest.mark.parametrize("net", NETS)
def test_eval_refusals(net):
    _refused(_fn(net, "eval_input")(P, P, 100, P, P, 128, *_bn(net), P, ST),
             "max_samples must be a positive multiple of 128")
    _refused(_fn(net, "eval_pool")(P, P, 256, P, P, -1, 128, P, *_bn(net), P, ST),
             "bad image range")


@pytest.mark.parametrize("net", NETS)
def test_end_epoch_refuses_a_null_output(net):
    _refused(_fn(net, "end_epoch")(P, None, ST), "null pointer")


@pytest.mark.parametrize("net", NETS)
def test_workspace_offset_refuses_an_unknown_id(net):
    off = ctypes.c_long()
    _refused(_fn(net, "workspace_offset")(99, 256, ctypes.byref(off)), "bad workspace id 99")


@pytest.mark.parametrize("net", NETS)
def test_workspace_offset_refuses_a_null_output(net):
    _refused(_fn(net, "workspace_offset")(0, 256, None), "null pointer")


def test_row_count_refusals():
    from flsim._lib import lib
    L = lib()
    text = "bad row count 100 (workspace 256)"
    _refused(L.flsim_vgg11_fwd_bwd_loaded_rows(P, P, 256, 100, P, P, SEED, 1, P, ST), text)
    _refused(L.flsim_vgg11_bn_fwd_bwd_loaded_rows(P, P, 256, 100, P, P, SEED, 1, P, P, ST), text)
    _refused(L.flsim_pn1_bwd_rows(P, P, 256, 100, P, 1, ST), text)


def test_pn1_passes_without_begin_epoch_are_refused():
    """No flsim_pn1_begin_epoch ran on the (fake) gradstate: its slab rows were never written."""
    from flsim._lib import lib
    L = lib()
    fwd = "forward rows without flsim_pn1_begin_epoch"
    bwd = "backward pass without flsim_pn1_begin_epoch on this gradstate"
    _refused(L.flsim_pn1_fwd_rows(P, P, 256, 0, P, P, P, 128, P, SEED, 1, P, ST), fwd)
    _refused(L.flsim_pn1_fwd_loaded_rows(P, P, 256, 0, 128, P, P, SEED, 1, P, ST), fwd)
    _refused(L.flsim_pn1_bwd_rows(P, P, 256, 128, P, 1, ST), bwd)
    _refused(L.flsim_pn1_fwd_bwd_chunk_async(P, P, 256, P, P, P, P, 4, P, 4, P, P, 1, 8, SEED, 1,
                                             P, ST), bwd)
    _refused(L.flsim_pn1_fwd_bwd_input_async(P, P, 256, P, P, P, 128, P, SEED, 1, P, ST), bwd)


def test_check_raises_value_error_with_the_message():
    from flsim._lib import check
    with pytest.raises(ValueError, match=r"^chunk of 256 samples exceeds workspace \(128\)$"):
        check(chunk("pn1", max_samples=128, n_chunk=2))
