"""A free TCP port for the process groups of tests/test_distributed.py (CPU) and
tests/test_gpu_multirank.py.  A helper module, not a test; it imports neither torch nor the library."""
import socket


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p
