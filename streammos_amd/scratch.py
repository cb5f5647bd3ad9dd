"""Per-stream scratch buffers of the op wrappers and the engines: one key, one table type, one release.

A buffer belongs to (device index, HIP stream, namespace, tag).  Launches on different streams never share one; the same
stream reuses it in stream order from frame to frame.  The namespace separates work that is captured on ONE stream but
replayed concurrently on several (the TTA groups of StreamRunner(graph=True, split=k) are all captured on torch's capture
stream): each group is captured under a ``GraphNamespace`` of its own, so the groups' graphs do not share scratch.
"""
import collections
import contextlib
import weakref

import torch

# The two private torch._C entry points behind torch.cuda.current_stream(...).cuda_stream / torch.cuda.current_device(),
# resolved once; a torch build without them gets the public (slower: ~4 us + ~3 us per launch) calls instead.
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_raw_device = getattr(torch._C, "_cuda_getDevice", None)
if _raw_stream is None:
    def _raw_stream(index):
        return torch.cuda.current_stream(index).cuda_stream
if _raw_device is None:
    _raw_device = torch.cuda.current_device


def _dev_index(device):
    return device.index if device.index is not None else _raw_device()


def _stream(t):
    """raw handle of torch's current HIP stream on t's device (the C call behind torch.cuda.current_stream(...).cuda_stream:
    the wrapper objects cost ~4 us per launch on the host)."""
    return _raw_stream(_dev_index(t.device))


class _NoGuard:
    """`with` target for a launch on the device that is already current: nothing to switch, nothing to restore."""
    __slots__ = ()

    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


_NO_GUARD = _NoGuard()


def _on(device):
    """Device guard for a launch: torch.cuda.device(...) only where the tensor's device is not the current one (the usual
    one-process-per-GPU case never switches; the guard object and its two device queries cost ~3 us per launch)."""
    return _NO_GUARD if device.index is None or _raw_device() == device.index else torch.cuda.device(device)


Key = collections.namedtuple("Key", "device stream namespace tag")       # device: its index; stream: the raw HIP handle
# The namespace of scratch that is baked into a runner's captured graphs; eager work runs in namespace 0.
GraphNamespace = collections.namedtuple("GraphNamespace", "owner group")

_tables = weakref.WeakSet()             # every live Table: one that dies with its owner is never walked again
_namespace = 0
_owner_tokens = iter(range(1, 1 << 62))


def new_workspace_owner():
    """A token for GraphNamespace.owner that is never handed out twice (id(obj) can be: a later runner allocated at a freed
    runner's address would alias its namespaces)."""
    return next(_owner_tokens)


@contextlib.contextmanager
def namespace(ns):
    """Requests inside the block use namespace `ns`; the previous one is back afterwards, also after an exception."""
    global _namespace
    prev, _namespace = _namespace, ns
    try:
        yield
    finally:
        _namespace = prev


class Table:
    """{Key: flat buffer}.  ``shared`` serves the wrappers of ops.py; every InferenceEngine owns one for its blocks."""
    __slots__ = ("_bufs", "__weakref__")

    def __init__(self):
        self._bufs = {}
        _tables.add(self)

    def get(self, tag, shape, dtype, device, zero=False):
        """One flat buffer per key, grown to the largest request seen: consecutive frames on a stream reuse it in stream
        order instead of holding a fresh allocation per frame that the host has enqueued ahead of the GPU.  The returned
        view is valid until the next request with the same tag on the same stream (callers consume it within the frame).
        zero=True: zero-filled when (re)allocated -- for buffers whose users leave them zero.  A tag has one dtype."""
        index = device.index
        if index is None:
            index = _raw_device()
        key = (index, _raw_stream(index), _namespace, tag)      # a plain tuple finds a Key: the per-launch path builds no more
        need = 1
        for d in shape:
            need *= int(d)
        buf = self._bufs.get(key)
        if buf is not None and buf.dtype != dtype:
            raise RuntimeError("scratch %r holds %s, asked for %s" % (tag, buf.dtype, dtype))
        if buf is None or buf.numel() < need:
            buf = self._bufs[Key._make(key)] = (torch.zeros if zero else torch.empty)(need, dtype=dtype, device=device)
        return buf[:need].view(shape)

    def entries(self, tag=None):
        """[(Key, buffer)] of this table, or of one tag."""
        return [(key, buf) for key, buf in self._bufs.items() if tag is None or key.tag == tag]


shared = Table()


def entries(tag=None):
    """(Key, buffer) of every live table, or of one tag."""
    for table in list(_tables):
        yield from table.entries(tag)


def release(device=None, stream=None, owner=None):
    """Drops scratch of every live table: all of it, one device's or one HIP stream's eager scratch, or (owner = the token
    in a runner's GraphNamespace) exactly what that runner's captured graphs use.  Scratch baked into captured graphs is
    spared by a device / stream release: torch hands pooled streams to several runners, so a stream handle alone does not
    say whose scratch an entry is."""
    if device is not None and not isinstance(device, int):
        device = _dev_index(torch.device(device))
    for table in list(_tables):
        for key in list(table._bufs):
            graph = isinstance(key.namespace, GraphNamespace)
            if owner is not None:
                drop = graph and key.namespace.owner == owner
            elif graph and (device is not None or stream is not None):
                drop = False
            else:
                drop = (device is None or key.device == device) and (stream is None or key.stream == stream)
            if drop:
                del table._bufs[key]
