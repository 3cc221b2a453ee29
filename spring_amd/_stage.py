"""What every stage wrapper shares: the error check and the life of a context handle.  A stage module writes its own
calls on top."""
import ctypes as C

from . import _lib


class ReorderError(RuntimeError):
    """Raised where the reference throws std::runtime_error (call_template_functions.cpp:60)."""


def chk(rc):
    if rc != 0:
        raise ReorderError("%s (code %d)" % (_lib.lib().spring_reorder_last_error().decode(), rc))


class Stage:
    """A context of the C ABI made by <_prefix>_create(device, &handle) and freed by <_prefix>_destroy(handle);
    _Info is the structure its calls fill.  info is the last call's result as a dict, None after a failed call."""

    _prefix = None
    _Info = None

    def __init__(self, device: int = -1):
        self._L = _lib.lib()
        self._h = C.c_void_p()
        chk(self._fn("create")(device, C.byref(self._h)))
        self.info = None

    def _fn(self, name):
        return getattr(self._L, "%s_%s" % (self._prefix, name))

    def close(self):
        if self._h:
            self._fn("destroy")(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _run(self, name, *args):
        """<_prefix>_<name>(handle, *args, &info) -> info, which is also kept in self.info."""
        info = self._Info()
        self.info = None
        chk(self._fn(name)(self._h, *args, C.byref(info)))
        self.info = info.asdict()
        return self.info

    def get_info(self):
        """The info of the result the context holds (the library refuses when there is none)."""
        info = self._Info()
        chk(self._fn("get_info")(self._h, C.byref(info)))
        return info.asdict()
