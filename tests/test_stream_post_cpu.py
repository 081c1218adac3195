"""CPU suite: the host side of the session's post-processing chain -- dfe_stream_post_check (host only, no device) on a valid struct and
on every member it refuses, and the parsing of DepthEstimationAPI's post= keywords."""
import ctypes as C

import pytest

from tests.test_stream_cpu import params

E_ARG, E_SHAPE = -1, -2                                           # DFE_E_ARG, DFE_E_SHAPE (include/dfe.h)
NAN = float("nan")


def valid_post(**over):
    """every stage on, the bilinear splat: each member is read"""
    from depth_estimation_amd._lib import StreamPost

    o = StreamPost()
    o.consistency_tol, o.fill, o.fill_levels, o.median_k, o.median_sigma, o.temporal = 1.0, 1, 0, 5, 20.0, 1
    o.t_tol, o.t_wmax, o.t_decay, o.t_has_gain, o.t_gain, o.t_has_bias, o.t_bias = 0.5, 8.0, 0.9, 1, 1.0, 1, 0.0
    o.t_splat, o.t_ztol, o.t_quant, o.t_min_cover = 1, 0.5, 1024.0, 0.25
    for k, v in over.items():
        setattr(o, k, v)
    return o


def check(dfe, p, o):
    return dfe.lib().dfe_stream_post_check(None if p is None else C.byref(p), None if o is None else C.byref(o))


def test_post_struct_sizes_and_valid(dfe):
    from depth_estimation_amd._lib import StreamPost, StreamPostOut

    p, keep = params(dfe)
    assert valid_post().struct_size == C.sizeof(StreamPost) == 18 * 4
    assert StreamPostOut().struct_size == C.sizeof(StreamPostOut) == 8 + 9 * C.sizeof(C.c_void_p)
    assert check(dfe, p, valid_post()) == 0
    assert check(dfe, p, StreamPost()) == 0                        # nothing enabled
    assert check(dfe, p, valid_post(t_splat=0, t_quant=NAN, t_min_cover=7.0)) == 0   # the splat's members are read with the bilinear splat only
    assert check(dfe, p, valid_post(temporal=0, t_wmax=0.0, t_decay=0.0)) == 0       # ... and the filter's with the filter on
    assert check(dfe, p, valid_post(median_sigma=-1.0)) == 0       # unguided
    assert check(dfe, p, valid_post(consistency_tol=0.0)) == 0     # off


BAD = [("struct_size", 68), ("struct_size", 76), ("struct_size", 0), ("consistency_tol", -1.0), ("consistency_tol", NAN), ("fill", 2), ("fill_levels", -1),
       ("median_k", 4), ("median_k", 17), ("median_k", -1), ("temporal", 2), ("t_tol", -0.5), ("t_tol", NAN), ("t_wmax", 1e-7), ("t_wmax", float("inf")),
       ("t_wmax", NAN), ("t_decay", 0.0), ("t_decay", 1.5), ("t_decay", NAN), ("t_has_gain", 2), ("t_gain", NAN), ("t_bias", float("inf")), ("t_splat", 2),
       ("t_splat", -1), ("t_ztol", -1.0), ("t_ztol", float("inf")), ("t_quant", 0.0), ("t_quant", NAN), ("t_quant", float("inf")), ("t_min_cover", -0.1),
       ("t_min_cover", 1.5), ("t_min_cover", NAN)]


@pytest.mark.parametrize("member,value", BAD, ids=["%s=%r" % b for b in BAD])
def test_post_check_refuses(dfe, member, value):
    p, keep = params(dfe)
    assert check(dfe, p, valid_post(**{member: value})) == E_ARG
    text = dfe.lib().dfe_last_error(None).decode()
    assert "dfe_stream_post_check" in text and member in text, text   # the text names the entry and the member


def test_post_check_null_pointers_and_shapes(dfe):
    p, keep = params(dfe)
    assert check(dfe, None, valid_post()) == E_ARG
    assert check(dfe, p, None) == E_ARG
    assert check(dfe, None, None) == E_ARG
    p.maxh = 400                                                   # the window does not fit: dfe_stream_shapes' code comes through
    assert check(dfe, p, valid_post()) == E_SHAPE
    p, keep = params(dfe)
    p.extraction = 3                                               # ... and its argument errors
    assert check(dfe, p, valid_post()) == E_ARG


def test_python_post_keywords(dfe):
    sp = dfe.stream.stream_post
    o = sp(dict(consistency=1.5, fill=True, median=(5, 20.0), temporal=dict(tol=0.5, gain=1.25, splat="bilinear")))
    assert (o.consistency_tol, o.fill, o.fill_levels, o.median_k, o.median_sigma, o.temporal) == (1.5, 1, 0, 5, 20.0, 1)
    assert (o.t_tol, o.t_wmax, o.t_decay, o.t_has_gain, o.t_gain, o.t_has_bias, o.t_splat, o.t_ztol, o.t_quant, o.t_min_cover) == (0.5, 8.0, 1.0, 1, 1.25, 0, 1, 0.5, 1024.0,
                                                                                                                                  0.25)
    o = sp(dict(fill=3, median=7))
    assert (o.consistency_tol, o.fill, o.fill_levels, o.median_k, o.median_sigma, o.temporal) == (0.0, 1, 3, 7, 0.0, 0)
    o = sp({})
    assert (o.consistency_tol, o.fill, o.median_k, o.temporal) == (0.0, 0, 0, 0)
    p, keep = params(dfe)
    for good in (dict(consistency=1.5, fill=True, median=(5, 20.0), temporal=dict(tol=0.5, splat="bilinear")), dict(fill=3), {}):
        assert check(dfe, p, sp(good)) == 0                        # what the parser lets through, the library takes
    for bad in (dict(median=4), dict(median=17), dict(median=(5,)), dict(median=5.0), dict(median=True), dict(consistency=-1.0), dict(consistency=NAN),
                dict(fill=-1), dict(fill="yes"), dict(temporal=dict()), dict(temporal=dict(tol=-1.0)), dict(temporal=dict(tol=1.0, wmax=0.0)),
                dict(temporal=dict(tol=1.0, decay=0.0)), dict(temporal=dict(tol=1.0, splat="cubic")), dict(temporal=dict(tol=1.0, splat="bilinear", quant=0.0)),
                dict(temporal=dict(tol=1.0, key_channel=1)), dict(temporal=dict(tol=1.0, gain=(1.0, 2.0))), dict(temporal=dict(tol=1.0, speed=2)), dict(upsample=2), 5):
        with pytest.raises(ValueError):
            sp(bad)
    geometry = dict(hImg=120, wImg=160, maxh=16, maxw=16, output_extraction_method="mean")
    K = [[300, 0, 160], [0, 300, 120], [0, 0, 1]]
    with pytest.raises(ValueError):                                # both forms of the temporal filter
        dfe.DepthEstimationAPI(geometry, None, K, temporal=dict(tol=0.5), post=dict(temporal=dict(tol=0.5)))
    with pytest.raises(ValueError):
        dfe.DepthEstimationAPI(geometry, None, K, post=dict(median=6))
    api = dfe.DepthEstimationAPI(geometry, None, K, temporal=dict(tol=0.5), post=dict(fill=True))   # (the Python-side filter beside a chain without one)
    assert api.post.fill == 1 and api.temporal is not None
    assert dfe.DepthEstimationAPI(geometry, None, K).post is None
