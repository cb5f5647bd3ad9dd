"""streammos_amd/scratch.py and the switches of ops.py / engine.py on the host: CPU tensors, the two stream / device lookups
stubbed, an emptied registry of tables.  No GPU, no HIP library."""
import gc
import types
import weakref

import pytest
import torch

from streammos_amd import engine, ops, scratch
from streammos_amd.scratch import GraphNamespace, Key

CPU = torch.device("cpu")


@pytest.fixture
def where(monkeypatch):
    """The current (device index, stream handle) as two attributes a test sets; the registry holds the emptied shared table."""
    at = types.SimpleNamespace(device=0, stream=111)
    monkeypatch.setattr(scratch, "_raw_device", lambda: at.device)
    monkeypatch.setattr(scratch, "_raw_stream", lambda index: at.stream)
    monkeypatch.setattr(scratch, "_tables", weakref.WeakSet([scratch.shared]))
    monkeypatch.setattr(scratch.shared, "_bufs", {})
    return at


def _fill(table, at, device, tags):
    """The four kinds of entry for every tag on one device: eager, graph owner 7 group 0 and group 1, another stream."""
    at.device = device
    for tag in tags:
        at.stream = 111
        table.get(tag, (4,), torch.int32, CPU)
        for group in (0, 1):
            with scratch.namespace(GraphNamespace(7, group)):
                table.get(tag, (4,), torch.int32, CPU)
        at.stream = 222
        table.get(tag, (4,), torch.int32, CPU)


def test_release_stream_workspaces_filters_by_device_and_spares_graph_namespaces(where):
    """A (device, stream) release drops that device's eager scratch on that stream only -- another device's, another stream's
    and what is baked into a runner's captured graphs stay; the owner path drops exactly that runner's; no argument, all.
    Over the shared table (a flag word among its tags) and two engine-like tables on two devices."""
    e0, e1 = scratch.Table(), scratch.Table()
    for device in (0, 1):
        _fill(scratch.shared, where, device, ("stem_rows", "maxpool_flag"))
    _fill(e0, where, 0, (0, 1))
    _fill(e1, where, 1, (0, 1))

    def left():
        return {(name, key) for name, table in (("shared", scratch.shared), ("e0", e0), ("e1", e1)) for key, _ in table.entries()}
    everything = left()
    assert len(everything) == 2 * 2 * 4 + 2 * 4 + 2 * 4 and all(type(key) is Key for _, key in everything)
    assert {key for _, key in everything} == {key for key, _ in scratch.entries()}
    assert ("shared", Key(1, 111, GraphNamespace(7, 1), "maxpool_flag")) in everything

    ops.release_stream_workspaces(0, 111)
    gone = {(name, key) for name, key in everything if key.device == 0 and key.stream == 111 and key.namespace == 0}
    assert gone == {("shared", Key(0, 111, 0, "stem_rows")), ("shared", Key(0, 111, 0, "maxpool_flag")),
                    ("e0", Key(0, 111, 0, 0)), ("e0", Key(0, 111, 0, 1))}
    assert left() == everything - gone
    where.device = 1
    ops.release_stream_workspaces(torch.device("cpu"), 222)             # a device object: its index (here the current one's)
    gone |= {(name, key) for name, key in everything if key.device == 1 and key.stream == 222}
    assert left() == everything - gone and len(gone) == 8

    with scratch.namespace(GraphNamespace(8, 0)):                       # another runner's graphs, same device and stream
        where.device, where.stream = 0, 111
        scratch.shared.get("maxpool_flag", (4,), torch.int32, CPU)
    ops.release_stream_workspaces(owner=7)
    other = ("shared", Key(0, 111, GraphNamespace(8, 0), "maxpool_flag"))
    assert left() == {(name, key) for name, key in everything - gone if key.namespace == 0} | {other}
    assert len(left()) == 32 - 8 - 16 + 1

    ops.release_stream_workspaces()
    assert left() == set() and list(scratch.entries()) == []


def test_a_dead_table_is_not_walked_and_keeps_nothing_alive(where):
    table = scratch.Table()
    buf = table.get(0, (8,), torch.float32, CPU)
    ref = weakref.ref(buf._base if buf._base is not None else buf)
    assert len(list(scratch.entries())) == 1 and ref() is not None
    del table, buf
    gc.collect()
    assert ref() is None and list(scratch.entries()) == [] and list(scratch._tables) == [scratch.shared]
    scratch.release()                                                   # walks the shared table alone


def test_namespace_restores_the_previous_one(where):
    tags = iter(range(100))

    def used():
        """the namespace a request lands in now"""
        before = {key for key, _ in scratch.shared.entries()}
        scratch.shared.get(next(tags), (1,), torch.uint8, CPU)
        (key,) = {key for key, _ in scratch.shared.entries()} - before
        return key.namespace
    a, b = GraphNamespace(1, 0), GraphNamespace(1, 1)
    assert used() == 0
    with scratch.namespace(a):
        assert used() == a
        with scratch.namespace(b):
            assert used() == b
        assert used() == a                                              # nested two deep: back to the outer one
        with pytest.raises(ZeroDivisionError):
            with scratch.namespace(b):
                raise ZeroDivisionError
        assert used() == a                                              # after an exception
    assert used() == 0                                                  # after a normal exit


def test_get_grows_zeroes_and_holds_a_tag_to_one_dtype(where):
    table = scratch.Table()
    big = table.get("t", (6, 4), torch.float32, CPU)
    assert tuple(big.shape) == (6, 4) and big.is_contiguous()
    small = table.get("t", (5,), torch.float32, CPU)
    assert tuple(small.shape) == (5,) and small.data_ptr() == big.data_ptr()           # a view of the same storage
    assert [buf.numel() for _, buf in table.entries("t")] == [24]
    bigger = table.get("t", (25,), torch.float32, CPU)
    assert [buf.numel() for _, buf in table.entries("t")] == [25] and bigger._base is not big._base     # re-allocated
    assert table.entries() == table.entries("t") and table.entries("u") == []
    with pytest.raises(RuntimeError, match="holds torch.float32"):
        table.get("t", (2,), torch.int32, CPU)
    z = table.get("z", (7,), torch.int32, CPU, zero=True)
    assert not z.any()
    z.fill_(5)
    assert table.get("z", (7,), torch.int32, CPU, zero=True).eq(5).all()               # kept as its users left it
    assert not table.get("z", (9,), torch.int32, CPU, zero=True).any()                 # zero again when re-allocated
    where.stream = 222                                                                 # another stream: another buffer
    assert table.get("z", (9,), torch.int32, CPU, zero=True).data_ptr() != z.data_ptr() and len(table.entries("z")) == 2


_ROWS = [("is_deterministic", "set_deterministic", "SMOS_DETERMINISTIC", False),
         ("point_mlp_fused", "set_point_mlp_fused", "SMOS_POINT_MLP", False),
         ("point_head_fused", "set_point_head_fused", "SMOS_POINT_HEAD_TRAIN", False),
         ("conv1_fused", "set_conv1_fused", "SMOS_CONV1_TRAIN", False),
         ("bilinear_bwd_own", "set_bilinear_bwd_own", "SMOS_BILINEAR_BWD", True)]
_OFF = ("0", "false", "off", "no", " OFF ", "False", "No\n")
_ON = ("1", "true", "on", "yes", "2", " 1 ", "x")
_UNSET = (None, "", "  ")


def test_env_on_spellings():
    assert [ops.env_on(v) for v in _OFF] == [False] * len(_OFF)
    assert [ops.env_on(v) for v in _ON] == [True] * len(_ON)
    assert [ops.env_on(v) for v in _UNSET] == [None] * len(_UNSET)


@pytest.mark.parametrize("name,setter,var,default", _ROWS)
def test_switch_resolution(monkeypatch, name, setter, var, default):
    switch, set_ = getattr(ops, name), getattr(ops, setter)
    assert type(switch) is ops.Switch and switch.var == var and switch.default is default and set_ == switch.set
    monkeypatch.setattr(torch, "are_deterministic_algorithms_enabled", lambda: False)
    monkeypatch.delenv(var, raising=False)
    prev = set_(None)
    try:
        assert switch() is default                                      # nothing set anywhere
        for text in _OFF + _ON + _UNSET[1:]:                            # the environment, read on every call
            monkeypatch.setenv(var, text)
            assert switch() is (default if text in _UNSET else text in _ON), text
        monkeypatch.setenv(var, "1")
        assert set_(False) is None and switch() is False                # the explicit setting goes first
        monkeypatch.setenv(var, "0")
        assert set_(True) is False and switch() is True
        assert set_(None) is True and switch() is False                 # None hands the decision back
        assert set_(1) is None and set_(None) is True                   # stored as a bool
        monkeypatch.delenv(var)
        assert switch() is default
        if switch.fallback is not None:                                 # asked where neither of the two speaks, at call time
            monkeypatch.setattr(torch, "are_deterministic_algorithms_enabled", lambda: True)
            assert switch() is True
            monkeypatch.setenv(var, "off")
            assert switch() is False
    finally:
        set_(prev)


@pytest.mark.parametrize("attr,var,default,kind", engine.SWITCHES + engine.TRAIN_SWITCHES)
def test_read_switches_rows(monkeypatch, attr, var, default, kind):
    """Unset / "0" / "1" as before there was one spelling rule (bool rows: v != "0"; int rows: int(v)); the other spellings of
    a bool row by ops.env_on."""
    def read(text):
        if text is None:
            monkeypatch.delenv(var, raising=False)
        else:
            monkeypatch.setenv(var, text)
        obj = types.SimpleNamespace()
        engine.read_switches(obj, ((attr, var, default, kind),))
        return getattr(obj, attr)
    assert read(None) == default and type(read(None)) is type(default)
    if kind == "int":
        assert (read("0"), read("1"), read("7")) == (0, 1, 7) and type(read("1")) is int
        return
    assert read("0") is False and read("1") is True
    for text in _OFF:
        assert read(text) is False, text
    for text in _ON:
        assert read(text) is True, text
    for text in _UNSET:
        assert read(text) is default, text
