"""depth_estimation_amd -- host-side mirror of the reference's operator interface for the dense
patch-correlation flow->depth hot path, over the C ABI of libdfe.so (include/dfe.h).

The reference's host language is Lua/Torch7 (absent from the build image), so this mirror is
Python: same names, argument order and error behaviour as the Lua modules / functions it stands
in for (cited per symbol), with torch CUDA tensors playing the role of Torch7 tensors.  torch is
plumbing only (device memory, streams); every computation goes through libdfe.so, and there is
no CPU fallback -- a missing library or device raises.

    nn.SpatialMatching / nn.SpatialRadialMatching     (nnx modules used by the reference)
    extractoutput.extractOutput / extractOutputMarginalized   (extract_output.cpp)
    x2yx, yx2x, yx2xMulti, x2yxMulti, x2yxMulti2, getMiddleIndex, getOutputConfidences,
    processOutput                                       (opticalflow_model*.lua)
    unfold, compute_cartesian_groundtruth_cross_correlation  (radial/radial_opticalflow_groundtruth.lua)
    nn.CascadingAddTable, getModelMultiscale            (CascadingAddTable.lua, opticalflow_model_multiscale.lua)
    getC2PMask, getP2CMask, cartesian2polar, flow2depth (radial/cartesian2polar.lua, radial_opticalflow_display.lua)
    torch7_io.load / save, load_calibration             (Torch7 binary files: *.cal, saveModel / saveNetwork weights)
    saveModel, loadModel, loadWeightsFrom, saveNetwork, loadTesterNetwork, loadTrainerNetwork   (opticalflow_model_io.lua, radial_opticalflow_network.lua)
    prepareInput, rgb2y                                 (opticalflow_model.lua:131-151)
    version2.getNetwork, getTrainerNetwork, decodeFlow, flowPair   (version2/network.lua, version2/test.lua)
    flowDepthPair, refineFlowSubpixel                   (not in the reference: the single-scale step in one call, and its
                                                        opt-in sub-pixel flow -- subpixel.py)
    flowDepthPair(..., consistency=tol, gate=False), flowConsistency   (not in the reference: the step in both directions with a
                                                        forward-backward occlusion mask (subpixel.py), and that check on any two flow fields (fields.py))
    flowDepthPair(..., fill=True), fillHoles            (not in the reference: the rejected pixels filled from the kept ones by a
                                                        confidence-weighted push-pull (subpixel.py), and that operator on any planes (fields.py))
    flowDepthPair(..., median=k | (k, sigma)), weightedMedian   (not in the reference: the flow through a confidence-weighted median
                                                        guided by the first frame (subpixel.py), and that operator on any planes (fields.py))
    guidedUpsample                                      (not in the reference: a flow or depth field back at the camera's resolution by joint
                                                        bilateral upsampling with a confidence plane, holes skipped, motion boundaries
                                                        kept by the frame itself -- fields.py)
    forwardWarp, temporalFuse, temporalStep, TemporalFilter, DepthEstimationAPI(..., temporal=dict(tol=...))   (not in the reference: a
                                                        depth field carried along its own flow to the next frame's grid under a z-buffer and
                                                        fused with that frame's measurement, weights counting observations -- fields.py,
                                                        temporal.py, stream.py)
    forwardSplat, temporalStep(..., splat="bilinear"), TemporalFilter(..., splat="bilinear")   (not in the reference: the sub-pixel
                                                        forward warp, every source spread over four pixels and summed in integers,
                                                        reproducible bit for bit -- fields.py, temporal.py)
    radialFlowDepth(..., subpixel=True), refineRadialFlowSubpixel   (not in the reference: sub-pixel radial flow -- radial.py)
    radialFlowDepth(..., sgm=(P1, P2)), semiGlobalAggregate         (not in the reference: the radial cost volume summed along 4 or 8 image
                                                        directions under two label-change penalties before the arg-min, the polar columns
                                                        a ring -- radial.py)
    censusTransform, censusCostVolume, censusFlow, censusFlowDepthPair   (not in the reference: the census matching cost -- patch
                                                        signatures, Hamming distances summed over a small box, the first minimum -- for
                                                        frame pairs whose exposure differs; the one call returns flowDepthPair's keys -- census.py)
    semiGlobalAggregatePlane, censusFlowDepthPair(..., sgm=(P1, P2))     (not in the reference: the aggregation on the two-dimensional
                                                        label plane of a Cartesian matcher's [H][W][hWin][wWin] volume, its first customer
                                                        the census cost -- sgm_plane.py)
    semiGlobalPick, flowDepthPair(..., sgm=(P1, P2))    (not in the reference: a uniqueness confidence and a sub-pixel flow read off the
                                                        aggregate, and the SSD step through it in one call -- sgm_plane.py, subpixel.py)
    censusRadialCostVolume, censusRadialFlow, censusRadialFlowDepth     (not in the reference: the census cost down the polar rows with a
                                                        box whose columns are a ring -- the radial path for frame pairs whose exposure
                                                        differs, with no trained weights -- census_radial.py)
    MultiscaleModel.forwardFlow(..., census=True), censusPyramidScaleVolume   (not in the reference: the census cost in the raw-patch pyramid
                                                        matcher -- multiscale flow for frame pairs whose exposure differs, with no trained
                                                        weights -- multiscale.py, census.py)
    censusRefineSubpixel, censusFlow / censusFlowDepthPair(..., refine=True), forwardFlow(..., census=dict(refine=True))
                                                        (not in the reference: sub-pixel flow on the raw census cost, the vee fit through
                                                        the chosen cell's cost and its neighbours' -- census.py, multiscale.py)
    getModel(geometry).forwardFlow                      (a trained single-scale model per frame pair in one call,
                                                        output_extraction_method 'max' or 'mean' -- network.py)
    imageScale, DepthEstimationAPI(...).nextFrameDepth  (image.scale; depth_estimation_api.lua:134-198, video -> depth per camera
                                                        frame over the library's stream object -- stream.py)
    DepthEstimationAPI(..., post=dict(consistency=tol, fill=True | levels, median=k | (k, sigma), temporal=dict(tol=...)))
                                                        (not in the reference: the forward-backward check, hole filling, the guided median
                                                        and the temporal filter behind the pair step INSIDE the stream object, the filter's
                                                        state on the device -- last["flow_post"], weight_post, consistent, depth_post,
                                                        depth_post_conf, depth_fused, depth_fused_weight, depth_fused_flag -- stream.py)
"""
from ._lib import lib, DfeError, LIB_PATH  # noqa: F401
from .context import Context, get_ctx  # noqa: F401
from . import nn  # noqa: F401
from . import network, radial, glue, sfm2  # noqa: F401
from . import extractoutput  # noqa: F401
from .opticalflow_model import (  # noqa: F401
    x2yx,
    yx2x,
    centered2onebased,
    onebased2centered,
    yx2xMulti,
    x2yxMulti,
    x2yxMulti2,
    x2yxMultiNumber,
    getMiddleIndex,
    getOutputConfidences,
    getOutputConfidences2,
    processOutput,
    prepareInput,
    rgb2y,
)
from . import version2  # noqa: F401
from .subpixel import flowDepthPair, refineFlowSubpixel  # noqa: F401
from .fields import flowConsistency, fillHoles, weightedMedian, guidedUpsample, forwardWarp, forwardSplat, temporalFuse, temporalStep  # noqa: F401
from .temporal import TemporalFilter  # noqa: F401
from .sgm_plane import semiGlobalAggregatePlane, semiGlobalPick  # noqa: F401
from .census import censusTransform, censusCostVolume, censusFlow, censusFlowDepthPair, censusPyramidScaleVolume, censusRefineSubpixel  # noqa: F401
from .multiscale import CascadingAddTable, MultiscaleModel, MultiscalePrefilter, getModelMultiscale, getMultiscalePrefilter  # noqa: F401
from .network import getFilter, getFilterRadial, getModel, tables_random  # noqa: F401
from .radial import (getRMax, getC2PMask, getP2CMask, cartesian2polar, flow2depth, getKOutput, getP2CMaskOF,  # noqa: F401
                     computeDepthMapFromFlow, getTesterNetwork, getTrainerNetwork, getMatcher, radialFlowDepth, radial_out_shape, refineRadialFlowSubpixel,
                     semiGlobalAggregate)
from .census_radial import censusRadialCostVolume, censusRadialFlow, censusRadialFlowDepth  # noqa: F401
from .glue import SmartReshape, FunctionWrapper, Mul2, Log2, OutputExtractor, postProcessImage, enlargeMask  # noqa: F401
from . import stream  # noqa: F401
from .stream import imageScale, DepthEstimationAPI  # noqa: F401
from . import torch7_io, model_io  # noqa: F401
from .model_io import (saveModel, loadModel, loadWeightsFrom, saveNetwork, loadTesterNetwork, loadTrainerNetwork, copyWeights)  # noqa: F401
from .torch7_io import load_calibration  # noqa: F401
from .groundtruth import (  # noqa: F401
    unfold,
    cross_correlation_pad_output,
    compute_cartesian_groundtruth_cross_correlation,
)
