"""Plumbing of tests/test_gpu_guarded_replica_stream.py that is not what it guards: waiting for a stream and giving it back."""
from fcn_object_detector_amd import lib as L


def finish(stream: int) -> None:
    L.call("fcn_stream_sync", stream)


def give_back(stream: int) -> None:
    L.call("fcn_stream_destroy", stream)
