import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: test requires an MI355X GPU")


def pytest_collection_modifyitems(config, items):
    try:
        import parsec_amd as pm
        has_gpu = pm.hip_device_count() > 0
    except Exception:
        has_gpu = False
    if has_gpu:
        return
    skip = pytest.mark.skip(reason="no GPU visible")
    for item in items:
        if "gpu" in item.keywords:
            item.add_marker(skip)


@pytest.fixture(scope="module")
def ctx():
    import parsec_amd as pm
    c = pm.Context(nworkers=2, rank=0, world=1)
    yield c
    del c


_port_locks = []  # flock fds held for the session lifetime
_port_cache = {}  # salt -> base: repeat calls must return the same base


PORT_SLOT = 128  # ports per reservable window


def _lock_slot(path):
    """Session-lifetime exclusive flock on `path`; OSError if it is held.
    Opened read-only (flock needs no write access), so a lock file that a
    session of another user left behind can be taken again."""
    import fcntl
    try:
        fd = os.open(path, os.O_RDONLY)
    except FileNotFoundError:
        fd = os.open(path, os.O_RDONLY | os.O_CREAT, 0o644)
    try:
        fcntl.flock(fd, fcntl.LOCK_EX | fcntl.LOCK_NB)
    except OSError:
        os.close(fd)
        raise
    return fd


def port_base(salt=0, span=64):
    """A base with `span` (<= PORT_SLOT) consecutive bindable ports. Two
    safeguards: ports stay BELOW the ephemeral range (32768+, where
    outgoing sockets land), and the chosen window is reserved via a
    session-lifetime flock so concurrent test sessions on one host never
    pick overlapping windows (probing alone races: both sessions can see
    the same window free before either binds). Windows are whole
    PORT_SLOT-aligned slots with one lock file per slot, so two windows
    either are the same slot or share no port."""
    import socket
    if salt in _port_cache:
        return _port_cache[salt]
    assert span <= PORT_SLOT, span
    NSLOTS = 12000 // PORT_SLOT  # slots within 20000..31999
    start = (os.getpid() * 131 + salt * 977) % NSLOTS
    for attempt in range(NSLOTS):
        base = 20000 + ((start + attempt) % NSLOTS) * PORT_SLOT
        try:
            lf = _lock_slot(f"/tmp/.pa_test_slot_{base}.lock")
        except OSError:
            continue
        ok = True
        socks = []
        try:
            for off in range(span):
                sk = socket.socket(socket.AF_INET, socket.SOCK_STREAM)
                sk.setsockopt(socket.SOL_SOCKET, socket.SO_REUSEADDR, 1)
                try:
                    sk.bind(("127.0.0.1", base + off))
                except OSError:
                    ok = False
                    sk.close()
                    break
                socks.append(sk)
        finally:
            for sk in socks:
                sk.close()
        if ok:
            _port_locks.append(lf)  # released automatically at exit
            _port_cache[salt] = base
            return base
        os.close(lf)  # releases the flock; window is occupied anyway
    raise RuntimeError("no free port range found")
