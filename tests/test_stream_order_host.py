"""No GPU: the seam the stream-order tests (test_gpu_stream_order.py) depend on.  Every piece of side-stream work in ops.py
goes through ops._on_side, where SIDE_LAUNCH_HOOK can hold the side stream back; side work that entered a stream some other
way would not be delayed by the tests and so would not be tested."""
import ast
import os

import pytest

import stream_delay

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_launch_hook_is_unset_after_import():
    from boxsegliver_amd import ops
    assert ops.SIDE_LAUNCH_HOOK is None


def _dotted(node):
    parts = []
    while isinstance(node, ast.Attribute):
        parts.append(node.attr)
        node = node.value
    if isinstance(node, ast.Name):
        parts.append(node.id)
    return ".".join(reversed(parts))


def test_streams_are_entered_and_waited_for_in_the_seam_only():
    """torch.cuda.stream( and .wait_stream( occur only inside _on_side and side_join."""
    path = os.path.join(ROOT, "boxsegliver_amd", "ops.py")
    with open(path) as f:
        tree = ast.parse(f.read(), path)
    found = []

    for top in tree.body:                                      # owner = the module-level function or class the call sits in
        owner = getattr(top, "name", None)
        for node in ast.walk(top):
            if isinstance(node, ast.Call):
                name = _dotted(node.func)
                if name == "torch.cuda.stream":
                    found.append((owner, name))
                elif name.split(".")[-1] == "wait_stream":
                    found.append((owner, "wait_stream"))
    assert found, "the walk found no stream call at all"
    assert set(f for f, _ in found) == {"_on_side", "side_join"}, found
    assert sorted(found) == [("_on_side", "torch.cuda.stream"), ("_on_side", "wait_stream"), ("side_join", "wait_stream")], found


def test_hold_refuses_more_than_the_cap():
    with pytest.raises(ValueError):
        stream_delay.hold(None, stream_delay.CAP_MS + 1)
    with pytest.raises(ValueError):
        stream_delay.hold(None, -1.0)
    with pytest.raises(AssertionError):
        stream_delay.delay_for(stream_delay.CAP_MS / stream_delay.FACTOR + 1.0)
    assert stream_delay.delay_for(1.0) == stream_delay.MIN_MS and stream_delay.delay_for(30.0) == 120.0
