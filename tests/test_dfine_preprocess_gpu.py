"""GPU tests of the D-FINE image pre-processing: dfine.preprocess_images (csrc/dfine_preprocess.hip) against the installed
RTDetrImageProcessorPil, for bits; and the processor bound by dfine.bind_processor.  No test provokes a fault: tables out of
range are exercised on the host only (test_dfine_preprocess_host.py)."""
import functools

import numpy as np
import pytest
import torch

import dfine_preprocess_ref as ref

pytestmark = pytest.mark.gpu

CASES = ref.cases()


def _processor_class():
    import transformers
    return transformers.RTDetrImageProcessorPil


@functools.lru_cache(maxsize=None)
def _processor(out_h, out_w):
    return _processor_class()(size={"height": out_h, "width": out_w})


def _pixel_values(images, size):
    return _processor(*size)(images=list(images), return_tensors="pt")["pixel_values"]


@functools.lru_cache(maxsize=None)
def _expected(name):
    from PIL import Image
    img, size = CASES[name]
    return _pixel_values([Image.fromarray(img)], size)


@functools.lru_cache(maxsize=None)
def _frames_640():
    """three sources of the sizes the scripts meet, and the processor's output for each, computed once"""
    imgs = [ref.noise(480, 700, 21), ref.noise(1080, 1920, 22), ref.noise(640, 640, 23)]
    return imgs, _pixel_values(imgs, (640, 640))


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_host_case_equals_the_processor_bit_for_bit(name, cuda_device):
    from PIL import Image
    from defectdetection_viaobjectdetection_amd import dfine
    img, size = CASES[name]
    want = _expected(name)
    for image in (img, Image.fromarray(img)):
        got = dfine.preprocess_images([image], size)
        assert got.is_cuda and got.dtype == torch.float32 and got.is_contiguous() and got.shape == want.shape
        assert torch.equal(got.cpu(), want)


def test_mixed_sizes_at_640_go_through_one_set_of_launches(cuda_device):
    from defectdetection_viaobjectdetection_amd import dfine
    imgs, want = _frames_640()
    got = dfine.preprocess_images(imgs, (640, 640))
    assert got.shape == (3, 3, 640, 640) and torch.equal(got.cpu(), want)
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        dfine.preprocess_images(imgs, (640, 640))
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    assert sum("dfine_pre_h_kernel" in n for n in names) == 1 and sum("dfine_pre_v_kernel" in n for n in names) == 1, names
    assert len(names) <= 3, names   # the two launches and the one upload


def test_one_frame_and_five_frames_of_one_size(cuda_device):
    from defectdetection_viaobjectdetection_amd import dfine
    imgs, want = _frames_640()
    assert torch.equal(dfine.preprocess_images([imgs[0]], (640, 640)).cpu(), want[:1])
    small = [ref.noise(37, 53, 30 + i) for i in range(5)]
    assert torch.equal(dfine.preprocess_images(small, (32, 48)).cpu(), _pixel_values(small, (32, 48)))
    same = [ref.noise(32, 48, 40 + i) for i in range(5)]   # no pass at all: one launch, a copy through the rescale table
    assert torch.equal(dfine.preprocess_images(same, {"height": 32, "width": 48}).cpu(), _pixel_values(same, (32, 48)))


def test_a_frame_does_not_depend_on_its_position_or_neighbours(cuda_device):
    from defectdetection_viaobjectdetection_amd import dfine
    names = [n for n in sorted(CASES) if CASES[n][1] == (32, 48)]
    frame = CASES["row_not_16_bytes"][0]
    others = [CASES[n][0] for n in names if n != "row_not_16_bytes"]
    alone = dfine.preprocess_images([frame], (32, 48))
    first = dfine.preprocess_images([frame] + others, (32, 48))
    last = dfine.preprocess_images(others + [frame], (32, 48))
    assert torch.equal(alone[0], first[0]) and torch.equal(alone[0], last[-1])
    assert torch.equal(first[1:], last[:-1])
    assert torch.equal(first.cpu(), torch.cat([_expected("row_not_16_bytes")] + [_expected(n) for n in names if n != "row_not_16_bytes"]))


def test_two_identical_calls_give_equal_bits(cuda_device):
    from defectdetection_viaobjectdetection_amd import dfine
    imgs, _ = _frames_640()
    a = dfine.preprocess_images(imgs, (640, 640))
    b = dfine.preprocess_images(imgs, (640, 640))
    assert a.data_ptr() != b.data_ptr() and torch.equal(a, b)


def test_back_to_back_calls_with_different_contents_are_both_right(cuda_device):
    """the second call refills the staging buffer the first one's upload reads: neither may see the other's bytes"""
    from defectdetection_viaobjectdetection_amd import dfine
    first = [ref.noise(480, 700, 50 + i) for i in range(4)]
    second = [ref.noise(480, 700, 60 + i) for i in range(4)]
    third = [ref.noise(300, 1000, 70)]                       # a smaller call reuses the front of the same buffers
    a = dfine.preprocess_images(first, (32, 48))
    b = dfine.preprocess_images(second, (32, 48))
    c = dfine.preprocess_images(third, (32, 48))
    assert torch.equal(a.cpu(), _pixel_values(first, (32, 48)))
    assert torch.equal(b.cpu(), _pixel_values(second, (32, 48)))
    assert torch.equal(c.cpu(), _pixel_values(third, (32, 48)))


def test_calls_on_two_streams_are_both_right(cuda_device):
    from defectdetection_viaobjectdetection_amd import dfine
    frames = [ref.noise(200, 300, 80 + i) for i in range(3)]
    want = _pixel_values(frames, (32, 48))
    side = torch.cuda.Stream()
    a = dfine.preprocess_images(frames[:2], (32, 48))
    with torch.cuda.stream(side):
        b = dfine.preprocess_images(frames[1:], (32, 48))
    c = dfine.preprocess_images(frames, (32, 48))
    torch.cuda.synchronize()
    assert torch.equal(a.cpu(), want[:2]) and torch.equal(b.cpu(), want[1:]) and torch.equal(c.cpu(), want)


def test_rescale_factor_and_images_outside_the_domain(cuda_device):
    from defectdetection_viaobjectdetection_amd import dfine
    img = CASES["upscale"][0]
    got = dfine.preprocess_images([img], (32, 48), rescale_factor=1 / 127.5)
    want = _processor_class()(size={"height": 32, "width": 48}, rescale_factor=1 / 127.5)(images=[img], return_tensors="pt")["pixel_values"]
    assert torch.equal(got.cpu(), want)
    assert torch.equal(got.cpu(), dfine.preprocess_images_torch([img], (32, 48), 1 / 127.5))
    for bad in ([np.zeros((200, 2, 3), np.uint8)], [np.zeros((20, 20, 3), np.float32)], []):
        with pytest.raises(ValueError):
            dfine.preprocess_images(bad, (32, 32))


def test_bound_processor_returns_pixel_values_on_the_device(cuda_device):
    from PIL import Image
    from defectdetection_viaobjectdetection_amd import dfine
    cls = _processor_class()
    plain, bound = cls(size={"height": 32, "width": 48}), dfine.bind_processor(cls(size={"height": 32, "width": 48}))
    names = [n for n in sorted(CASES) if CASES[n][1] == (32, 48)]
    images = [Image.fromarray(CASES[n][0]) for n in names]
    want = plain(images=images, return_tensors="pt")
    before = dict(dfine.preprocess_calls)
    got = bound(images=images, return_tensors="pt")
    assert dfine.preprocess_calls["kernel"] == before["kernel"] + 1 and dfine.preprocess_calls["original"] == before["original"]
    assert type(got) is type(want) and list(got.keys()) == list(want.keys()) == ["pixel_values"]
    pv = got["pixel_values"]
    assert pv.is_cuda and pv.dtype == torch.float32 and torch.equal(pv.cpu(), want["pixel_values"])
    moved = got.to(cuda_device)                                  # the scripts' .to(device) is a no-op
    assert moved["pixel_values"].data_ptr() == pv.data_ptr()
    assert pv.to(cuda_device).data_ptr() == pv.data_ptr()
    one = bound(images=images[1], return_tensors="pt")["pixel_values"]   # a single image, as the predictors pass it
    assert one.is_cuda and torch.equal(one.cpu(), want["pixel_values"][1:2])
    # the size given at the call, as the processor's own kwargs allow
    big = bound(images=images[:2], return_tensors="pt", size={"height": 64, "width": 64})["pixel_values"]
    assert big.is_cuda and torch.equal(big.cpu(), plain(images=images[:2], return_tensors="pt", size={"height": 64, "width": 64})["pixel_values"])
    assert bound.to_dict() == plain.to_dict()


@pytest.mark.parametrize("name", sorted(ref.fallback_calls()))
def test_bound_processor_fallbacks_return_the_original_cpu_result(name, cuda_device):
    from defectdetection_viaobjectdetection_amd import dfine
    make, call, images = ref.fallback_calls()[name]
    cls = _processor_class()
    want = cls(**make)(images=images, **call)
    bound = dfine.bind_processor(cls(**make))
    before = dict(dfine.preprocess_calls)
    got = bound(images=images, **call)
    assert dfine.preprocess_calls["original"] == before["original"] + 1 and dfine.preprocess_calls["kernel"] == before["kernel"]
    assert type(got) is type(want) and ref.same_feature(got, want)
    pv = got["pixel_values"]
    assert not (isinstance(pv, torch.Tensor) and pv.is_cuda)
