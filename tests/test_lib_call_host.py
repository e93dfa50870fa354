"""CPU: the one guarded way from Python to the C ABI (ubdvss_amd/_lib.py: launch, call, require_gpu, static_handle) over a stub
library that records its calls, a recording device guard and a known stream per device; ON_STREAM against include/ubd.h."""
import contextlib
import os
import re

import pytest
import torch

from ubdvss_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV0, DEV1 = torch.device("cuda:0"), torch.device("cuda:1")
STREAMS = {DEV0: 0, DEV1: 0x5151}          # cuda:0 on the default stream, cuda:1 on one of its own


class _Stub:
    """stands for the loaded library: every ubd_* name is a function that logs (name, args) and returns ``rc``"""

    def __init__(self, log, rc=0):
        self.log, self.rc = log, rc

    def ubd_last_error(self):
        return b"stub says no"

    def __getattr__(self, name):
        if not name.startswith("ubd_"):
            raise AttributeError(name)

        def fn(*args):
            self.log.append(("call", name, args))
            return self.rc
        return fn


@pytest.fixture
def log(monkeypatch):
    events = []

    class _Stream:
        def __init__(self, device):
            self.cuda_stream = STREAMS[torch.device(device)]

    @contextlib.contextmanager
    def guard(device):
        events.append(("enter", device))
        yield
        events.append(("exit", device))

    monkeypatch.setattr(_lib, "load", lambda: _Stub(events))
    monkeypatch.setattr(torch.cuda, "current_stream", _Stream)
    monkeypatch.setattr(torch.cuda, "device", guard)
    monkeypatch.setattr(_lib, "_static_handles", {})
    return events


def test_launch_appends_the_devices_stream_inside_the_devices_guard(log):
    a, b = object(), object()
    assert "ubd_loss" in _lib.ON_STREAM
    _lib.launch("ubd_loss", DEV1, a, b)
    assert log == [("enter", DEV1), ("call", "ubd_loss", (a, b, STREAMS[DEV1])), ("exit", DEV1)]
    assert STREAMS[DEV1] != STREAMS[DEV0]
    del log[:]
    _lib.launch("ubd_loss", DEV1, a, stream=7)               # a stream the caller looked up already is passed on, not looked up again
    assert log == [("enter", DEV1), ("call", "ubd_loss", (a, 7)), ("exit", DEV1)]


def test_launch_raises_with_name_code_and_last_error(log, monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: _Stub(log, rc=-3))
    with pytest.raises(RuntimeError) as e:
        _lib.launch("ubd_forward", DEV1, 1)
    assert "ubd_forward" in str(e.value) and "-3" in str(e.value) and "stub says no" in str(e.value)
    assert str(e.value) == "ubd_forward failed (code -3): stub says no"
    assert [ev[0] for ev in log] == ["enter", "call"]         # the error leaves through the guard


def test_launch_refuses_an_entry_without_a_stream_before_anything_is_called(log, monkeypatch):
    def no_load():
        raise AssertionError("the library must not be touched")
    monkeypatch.setattr(_lib, "load", no_load)
    for name in ("ubd_create", "ubd_loss_workspace_bytes", "ubd_x"):
        with pytest.raises(ValueError, match=name):
            _lib.launch(name, DEV1, 1, 2)
    assert log == []


def test_call_guards_only_a_given_device(log, monkeypatch):
    _lib.call("ubd_comm_unique_id", "buf")
    assert log == [("call", "ubd_comm_unique_id", ("buf",))]
    del log[:]
    _lib.call("ubd_comm_init", "h", "buf", 0, 1, 0, device=DEV1)
    assert log == [("enter", DEV1), ("call", "ubd_comm_init", ("h", "buf", 0, 1, 0)), ("exit", DEV1)]
    del log[:]
    with pytest.raises(ValueError, match="ubd_loss"):           # an entry that takes a stream has one way in
        _lib.call("ubd_loss", 1)
    assert log == []
    monkeypatch.setattr(_lib, "load", lambda: _Stub(log, rc=5))
    with pytest.raises(RuntimeError, match=r"ubd_create failed \(code 5\): stub says no"):
        _lib.call("ubd_create", 1, 2)


def _header_entries():
    """include/ubd.h -> {name: parameter list} of every declaration, comments removed (the names as tests/test_abi.py takes them)"""
    src = open(os.path.join(ROOT, "include", "ubd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    return dict(re.findall(r"\b(ubd_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S))


def test_on_stream_is_the_headers_set():
    entries = _header_entries()
    assert sorted(entries) == sorted(_lib.SIGNATURES)          # the parse sees every declaration
    with_stream = {name for name, params in entries.items() if re.search(r"\bvoid\s*\*\s*stream\s*$", params.strip())}
    assert len(with_stream) == 33
    assert _lib.ON_STREAM == with_stream
    assert isinstance(_lib.ON_STREAM, frozenset) and _lib.ON_STREAM <= set(_lib.SIGNATURES)
    for name in _lib.ON_STREAM:                                 # and the table agrees: a status comes back, a pointer goes last
        res, args = _lib.SIGNATURES[name]
        assert res is _lib._i and args[-1] is _lib._vp, name


def test_static_handles_are_made_once_per_classes_and_device_and_destroyed_once(log):
    h = _lib.static_handle(2, DEV1)
    assert _lib.static_handle(2, DEV1) is h
    assert [ev[:2] for ev in log] == [("enter", DEV1), ("call", "ubd_create"), ("exit", DEV1)]
    cfg = log[1][2][0]._obj                                     # byref(UbdConfig)
    assert (cfg.c_in, cfg.n_classes, cfg.fml_compatible, cfg.dtype) == (1, 2, 1, _lib.UBD_F32)
    h0 = _lib.static_handle(2, DEV0)
    h3 = _lib.static_handle(3, DEV1)
    assert len({id(x) for x in (h, h0, h3)}) == 3
    assert [ev[1] for ev in log if ev[0] == "enter"] == [DEV1, DEV0, DEV1]
    assert sum(ev[:2] == ("call", "ubd_create") for ev in log) == 3
    del log[:]
    _lib.reset_static_handles()
    assert _lib._static_handles == {}
    destroyed = [ev[2][0] for ev in log if ev[:2] == ("call", "ubd_destroy")]
    assert len(log) == 3 and sorted(map(id, destroyed)) == sorted(map(id, (h, h0, h3)))
    del log[:]
    _lib.reset_static_handles()                                 # nothing is destroyed twice
    assert log == []


def test_require_gpu(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError) as e:
        _lib.require_gpu("X")
    assert "X needs an MI355X" in str(e.value) and "no CPU fallback" in str(e.value)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    assert _lib.require_gpu("X") is torch
