"""CPU: the host side of gradient accumulation -- the two command lines' --accumulation_steps, the training loops' grouping of
micro-batches (zero_grad on a group's first, step on its last or the loader's last, no_sync() around the others, the loss divided by
N) on a stub model / optimizer that records calls, and the C-ABI's refusals that need no device."""
import ctypes as C
import importlib.util
import os
import types

import pytest

from src.data.synthetic import make_batch, make_pretrain_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cli(name):
    spec = importlib.util.spec_from_file_location("kmb_accum_cli_" + name.replace(".", "_"), os.path.join(ROOT, "km-bart_amd", name))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    return cli


@pytest.mark.parametrize("name", ["vcg_train.py", "pretrain.py"])
def test_cli_parses_accumulation_steps(name, tmp_path):
    cli = _cli(name)
    base = ["--checkpoint_dir", str(tmp_path), "--model_config", "x.json", "--synthetic", "2"]
    assert cli.parse_args(base).accumulation_steps == 1
    assert cli.parse_args(base + ["--accumulation_steps", "4"]).accumulation_steps == 4
    for bad in ("0", "-2"):
        with pytest.raises(ValueError, match="accumulation_steps"):
            cli.parse_args(base + ["--accumulation_steps", bad])


class _Loss:
    def __init__(self, log, v, scale=1.0):
        self.log, self.v, self.scale = log, v, scale

    def item(self):
        assert self.scale == 1.0, "the reported loss is the unscaled one"
        self.log.append("item")
        return self.v

    def __truediv__(self, n):
        return _Loss(self.log, self.v, self.scale / n)

    def backward(self):
        self.log.append("backward/%g%s" % (1.0 / self.scale, "/nosync" if self.log.model.in_no_sync else ""))

    def detach(self):
        return self


class _Log(list):
    model = None


class _NoSync:
    def __init__(self, model):
        self.model = model

    def __enter__(self):
        self.model.in_no_sync = True

    def __exit__(self, *a):
        self.model.in_no_sync = False
        return False


class _Model:
    """records calls; `wrapped`: a data-parallel wrapper's surface (no_sync, .module owns accumulate_gradients)"""

    def __init__(self, log, wrapped=False, pretrain=False):
        self.log, self.in_no_sync, self.pretrain = log, False, pretrain
        log.model = self
        inner = types.SimpleNamespace(accumulate_gradients=lambda on=True: log.append("accumulate/%s" % bool(on)))
        if wrapped:
            self.module = inner
            self.no_sync = lambda: _NoSync(self)
        else:
            self.accumulate_gradients = inner.accumulate_gradients

    def train(self):
        self.log.append("train")

    def forward(self, **kw):
        self.log.append("forward")
        loss = _Loss(self.log, 1.5)
        return ({"loss": loss},) if self.pretrain else (loss,)


class _Opt:
    def __init__(self, log):
        self.log = log

    def zero_grad(self):
        self.log.append("zero_grad")

    def step(self):
        self.log.append("step")


def _expected(n_batches, n_accum, wrapped):
    out = []
    for i in range(n_batches):
        first = i % n_accum == 0
        last = i % n_accum == n_accum - 1 or i == n_batches - 1
        out.append("forward")
        if first:
            out.append("zero_grad")
        out.append("backward/%d%s" % (n_accum, "/nosync" if (wrapped and not last) else ""))
        if last:
            out.append("step")
    return out


@pytest.mark.parametrize("wrapped", [False, True])
@pytest.mark.parametrize("n_batches", [1, 5, 6])
@pytest.mark.parametrize("n_accum", [1, 2, 3])
def test_fine_tune_groups_micro_batches(n_accum, n_batches, wrapped):
    from src.training import fine_tune
    log, lines = _Log(), []
    b = make_batch(2, enc_len=16, dec_len=8, num_regions=3)
    logger = types.SimpleNamespace(info=lambda m, pad=False: lines.append(m))
    args = types.SimpleNamespace(amp=False, epochs=1, accumulation_steps=n_accum)
    mean = fine_tune(0, _Model(log, wrapped), [b] * n_batches, _Opt(log), "cpu", args, logger=logger)
    calls = [c for c in log if c != "item"]
    on = ["accumulate/True"] if n_accum > 1 else []
    off = ["accumulate/False"] if n_accum > 1 else []
    assert calls == on + ["train"] + _expected(n_batches, n_accum, wrapped) + off
    assert log.count("step") == -(-n_batches // n_accum) and log.count("zero_grad") == log.count("step")
    assert log.count("item") == n_batches and mean == 1.5                      # per micro-batch, the unscaled loss
    assert [ln.split(",")[1].strip() for ln in lines] == ["Step [%d/%d]" % (i + 1, n_batches) for i in range(n_batches)]


@pytest.mark.parametrize("n_accum,n_batches", [(1, 2), (2, 2), (3, 5)])
def test_pretrain_groups_micro_batches(n_accum, n_batches):
    from src.training import pretrain
    log = _Log()
    b = make_pretrain_batch(2, enc_len=16, dec_len=8, num_regions=3, num_labels=7, num_attributes=5, num_relations=3)
    args = types.SimpleNamespace(amp=False, epochs=1, accumulation_steps=n_accum)
    pretrain(0, _Model(log, True, pretrain=True), [b] * n_batches, _Opt(log), "cpu", args)
    calls = [c for c in log if c != "item"]
    on = ["accumulate/True"] if n_accum > 1 else []
    off = ["accumulate/False"] if n_accum > 1 else []
    assert calls == on + ["train"] + _expected(n_batches, n_accum, True) + off


def test_loops_refuse_what_cannot_accumulate():
    from src.training import fine_tune
    b = make_batch(2, enc_len=16, dec_len=8, num_regions=3)
    log = _Log()
    with pytest.raises(ValueError, match="accumulation_steps"):
        fine_tune(0, _Model(log), [b], _Opt(log), "cpu", types.SimpleNamespace(amp=False, epochs=1, accumulation_steps=0))
    assert log == []
    # a model without accumulate_gradients(): an error, never a loop that steps on the last micro-batch's gradients alone
    bare = types.SimpleNamespace(train=lambda: None, forward=lambda **kw: (_Loss(log, 1.0),))
    with pytest.raises(RuntimeError, match="accumulate_gradients"):
        fine_tune(0, bare, [b, b], _Opt(log), "cpu", types.SimpleNamespace(amp=False, epochs=1, accumulation_steps=2))
    assert "step" not in log
    # an error inside the loop is the one reported; accumulation is still switched off
    log = _Log()
    model = _Model(log)

    def boom(**kw):
        raise KeyError("boom")
    model.forward = boom
    with pytest.raises(KeyError, match="boom"):
        fine_tune(0, model, [b, b], _Opt(log), "cpu", types.SimpleNamespace(amp=False, epochs=1, accumulation_steps=2))
    assert log == ["accumulate/True", "train", "accumulate/False"]


def test_no_sync_makes_post_backward_a_no_op():
    """DistributedDataParallel.no_sync() on an instance built without a process group's machinery: inside it neither reducer entry
    touches anything (the `self.reducer` of this bare instance does not even exist); outside, the entries run again"""
    from kmbart.parallel import DistributedDataParallel
    ddp = DistributedDataParallel.__new__(DistributedDataParallel)
    assert ddp._no_sync is False
    with ddp.no_sync() as inner:
        assert inner is ddp and ddp._no_sync is True
        assert ddp._reduce() is None and ddp._reduce_native() is None
        with ddp.no_sync():
            pass
        assert ddp._no_sync is True          # nesting restores the outer state
    assert ddp._no_sync is False
    with pytest.raises(AttributeError):
        ddp._reduce()


def test_accumulation_needs_a_bound_stage():
    import __graft_entry__
    from kmbart import _lib
    from kmbart._lib import KmbConfig, check
    from test_cabi_cpu import VCG_BASE
    __graft_entry__.build()
    lib = _lib.load()
    h = C.c_void_p()
    check(lib.kmb_create(C.byref(KmbConfig(**VCG_BASE)), C.byref(h)))
    try:
        assert lib.kmb_set_grad_accumulation(h, 1) != 0 and b"stage" in lib.kmb_last_error()
        check(lib.kmb_set_grad_accumulation(h, 0))
        check(lib.kmb_zero_grad(h))
        n = lib.kmb_arena_elems(h)
        assert lib.kmb_bind_grad_stage(h, C.c_void_p(256), n - 1) != 0 and b"floats" in lib.kmb_last_error()
        assert lib.kmb_bind_grad_stage(h, C.c_void_p(260), n) != 0 and b"aligned" in lib.kmb_last_error()
        check(lib.kmb_bind_grad_stage(h, C.c_void_p(1 << 20), n))     # (an address only: nothing is launched here)
        check(lib.kmb_set_grad_accumulation(h, 1))
        assert lib.kmb_bind_grad_stage(h, None, 0) != 0 and b"off" in lib.kmb_last_error()
        check(lib.kmb_set_grad_accumulation(h, 0))
        check(lib.kmb_bind_grad_stage(h, None, 0))
        assert lib.kmb_set_grad_accumulation(h, 1) != 0
    finally:
        lib.kmb_destroy(h)
