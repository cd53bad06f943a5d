"""The ledger of guarded kernel entry points (no GPU).

Every `int fcn_*(` / `size_t fcn_*(` declared in include/fcnhip.h is in exactly one of three sets:
  guarded    its name occurs as a called entry point in a guard-banded test file (tests/test_gpu_guarded*.py,
             tests/test_gpu_f16_pointwise.py) - found by scanning those files, not listed by hand;
  NO_KERNEL  runtime, stream, event, graph, memory, collective and size / configuration queries: nothing to guard;
  PENDING    name -> why it has no guarded test yet.
A new entry point therefore needs a guarded test or a pending reason; a name that became guarded must leave the hand-written sets."""
import glob
import os
import re

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "fcnhip.h")
GUARDED_FILES = sorted(glob.glob(os.path.join(ROOT, "tests", "test_gpu_guarded*.py"))) + [os.path.join(ROOT, "tests", "test_gpu_f16_pointwise.py")]

NO_KERNEL = {
    # runtime, memory, streams, events, graphs
    "fcn_abi_version", "fcn_device_count", "fcn_init", "fcn_device_name", "fcn_device_sync", "fcn_malloc", "fcn_free", "fcn_host_malloc",
    "fcn_host_free", "fcn_memset_async", "fcn_memcpy_h2d_async", "fcn_memcpy_d2h_async", "fcn_memcpy_d2d_async", "fcn_stream_create",
    "fcn_stream_destroy", "fcn_stream_sync", "fcn_event_create", "fcn_event_destroy", "fcn_event_record", "fcn_event_sync",
    "fcn_event_elapsed_ms", "fcn_stream_wait_event", "fcn_graph_begin", "fcn_graph_end", "fcn_graph_launch", "fcn_graph_destroy",
    # collectives (RCCL)
    "fcn_comm_unique_id", "fcn_comm_init", "fcn_comm_allreduce_sum_f32", "fcn_comm_destroy",
    # size / configuration queries and plan bookkeeping that launch nothing
    "fcn_conv2d_num_configs", "fcn_conv2d_first_layer_config", "fcn_conv2d_config_lds_bytes", "fcn_conv2d_config_waves_k",
    "fcn_conv2d_wgrad_num_configs", "fcn_conv2d_wgrad_split_config", "fcn_detect_workspace_bytes",
    "fcn_score_masks_workspace_bytes",
}

PENDING: dict = {}


def declared():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)      # comments name entry points too
    return sorted(set(re.findall(r"^\s*(?:int|size_t)\s+(fcn_\w+)\s*\(", text, flags=re.M)))


def guarded(names):
    """Names that a guarded test file CALLS: by name as a string literal (`L.call("name", ...)`, also through a local helper that
    forwards the name) or as an attribute of the loaded library (`lib.name(...)`).  Comments and docstrings do not count."""
    called = set()
    for p in GUARDED_FILES:
        src = open(p).read()
        src = re.sub(r'''""".*?"""''', " ", src, flags=re.S)
        src = re.sub(r"#.*", " ", src)
        called |= set(re.findall(r"""["'](fcn_\w+)["']""", src)) | set(re.findall(r"\.(fcn_\w+)\s*\(", src))
    return {n for n in names if n in called}


def test_the_header_is_parsed():
    names = declared()
    assert len(names) >= 100 and "fcn_conv2d_fwd_group_f32" in names and "fcn_score_masks_workspace_bytes" in names
    assert "fcn_last_error_string" not in names      # (returns const char*: not an int / size_t entry point)


def test_every_entry_point_is_guarded_or_accounted_for():
    names = declared()
    g = guarded(names)
    missing = [n for n in names if n not in g and n not in NO_KERNEL and n not in PENDING]
    assert not missing, "entry points without a guarded test or a pending reason: %s" % missing


def test_the_hand_written_lists_are_not_stale():
    names = set(declared())
    g = guarded(names)
    assert not (NO_KERNEL | set(PENDING)) - names, "listed names that the header no longer declares: %s" % sorted((NO_KERNEL | set(PENDING)) - names)
    assert not NO_KERNEL & set(PENDING), "names in both hand-written sets: %s" % sorted(NO_KERNEL & set(PENDING))
    assert not set(PENDING) & g, "pending names that have a guarded test now: %s" % sorted(set(PENDING) & g)
    kernels_used_as_plumbing = {"fcn_device_sync", "fcn_memcpy_h2d_async", "fcn_memcpy_d2h_async", "fcn_init", "fcn_malloc", "fcn_free"}
    stale = (NO_KERNEL & g) - kernels_used_as_plumbing - {n for n in NO_KERNEL if n.startswith("fcn_conv2d_") or n.endswith("_bytes")}
    assert not stale, "no-kernel names that a guarded test calls: %s" % sorted(stale)
    assert all(isinstance(r, str) and len(r) > 20 for r in PENDING.values())


def test_the_hot_path_of_this_ledger_is_guarded():
    """What the half-float guarded file was written for stays guarded."""
    g = guarded(declared())
    for n in ("fcn_conv2d_group_prepare", "fcn_conv2d_fwd_group_f32", "fcn_conv2d_group_attach_tail", "fcn_conv2d_tail_scratch_bytes",
              "fcn_conv2d_tail_arrive_bytes", "fcn_maxpool_fwd_f16", "fcn_lrn_fwd_f16", "fcn_maxpool_lrn5_fwd_f16",
              "fcn_maxpool_lrn5_conv1x1_fwd_f16", "fcn_nchw_f32_to_nhwc_f16", "fcn_nhwc_f16_to_nchw_f32", "fcn_preprocess_bgr8_f16",
              "fcn_preprocess_bgr8_batch", "fcn_preprocess_bgr8_rois", "fcn_conv2d_wgrad_group_cfg_f32", "fcn_conv_weights_flip_batch_f32"):
        assert n in g, n


def test_the_byte_and_integer_kernels_stay_guarded():
    """What tests/test_gpu_guarded_{augment,scene,masks,detect}.py were written for stays guarded."""
    g = guarded(declared())
    for n in ("fcn_compose_scene_bgr8", "fcn_compose_scene_view_bgr8", "fcn_blur_gauss_bgr8", "fcn_blur_box_bgr8", "fcn_blur_median_bgr8",
              "fcn_color_augment_bgr8", "fcn_mask_to_label_f32", "fcn_score_masks", "fcn_detect_decode_group", "fcn_gen_targets",
              "fcn_gen_targets_nhwc"):
        assert n in g, n
    assert PENDING == {}
