"""stereo_match_amd — MI355X-native drop-in for the ocean1100/stereo_match hot path.

Public surface (mirrors the reference / OpenCV names the reference uses):

* :func:`compute_disparity` — ``stereo_vision/stereo_vision.py:132``
* :func:`StereoSGBM_create`, :func:`createRightMatcher` — the cv2 /
  cv2.ximgproc calls at ``stereo_vision/stereo_vision.py:153,171``
* :func:`parse_config_file` — ``disparity_calculation.py:75``
* :func:`rectify_opencv`, :func:`stereoRectify`, :func:`initUndistortRectifyMap`, :func:`remap`,
  :func:`cvtColor`, :class:`StereoRectifier` — the rectification front end,
  ``disparity_calculation.py:131-210,286-287``
* :func:`fastNlMeansDenoising` — the denoiser in front of the matcher in the test flow,
  ``disparity_test.py:94-95``
* :func:`image_measure`, :func:`gaussian_filter`, :func:`pyrDown` — the reference's own smoothing
  function (``disparity_test.py:54-66,82-83``: scipy's float64 Gaussian, bit for bit) and the
  ``cv2.pyrDown`` in front of ``try_try.py``'s matcher (``:56-57``)
* :func:`extract_point_cloud`, :func:`format_ply`, :func:`write_point_cloud` — the masked point
  cloud and its ASCII PLY file, the tail of every script (``disparity_calculation.py:302-320``)
* :func:`imwrite`, :func:`imencode_png`, :func:`imencode_png_batch`, :func:`imencode_png_host`,
  :func:`write_disparity_png`, :func:`encode_disparity_png` — PNG files (``cv2.imwrite``,
  ``disparity_calculation.py:247-291``) and the KITTI 16-bit disparity format, encoded on the device
* :func:`imread`, :func:`imdecode`, :func:`imdecode_batch`, :func:`imdecode_host`,
  :func:`read_disparity_png`, :func:`decode_disparity_png` — PNG files read back (``cv2.imread``,
  ``disparity_test.py:79-80``, ``mapTo3D.py:78-79``), decoded on the device
* :class:`McCnnFast` — the mc-cnn *fast* matching cost, images to the float32 cost volume of
  :meth:`StereoSGBM.computeFromCost` (``mc_cnn/script.py:9``, ``mapTo3D_mc_cnn.py:71``)
* :class:`McCnnAccurate` — the mc-cnn *accurate* matching cost (112-map features, a fully connected
  scorer and a sigmoid; ``mc_cnn/script.py:10``), the same volume for :class:`McCnnStereo`;
  ``precision="bf16"`` / ``with_precision("bf16")`` runs the scorer's hidden layers on the bfloat16
  matrix instruction in one fused kernel (opt-in; the default ``"f32"`` is unchanged)
* :class:`McCnnStereo`, :func:`mc_aggregate`, :func:`mc_disparity`, :class:`McCnnStereoParams` — mc-cnn's
  own stereo method on that volume: its SGM, left-right interpolation, sub-pixel step, median and
  bilateral filter, up to the disparity maps ``mapTo3D_mc_cnn.py:70-77`` reads;
  :class:`McCnnCrossParams`, :func:`mc_cross_aggregate`, :func:`mc_cross_arms` — its cross-based cost
  aggregation, off unless ``McCnnStereo(..., cross=...)`` asks for it

All compute runs in ``libstereo_match_amd.so`` (HIP, gfx950) through the
C-ABI in ``include/stereo_match_amd.h``; there is no CPU fallback.
"""
from .matcher import (STEREO_SGBM_MODE_HH, STEREO_SGBM_MODE_HH4, STEREO_SGBM_MODE_SGBM,
                      STEREO_SGBM_MODE_SGBM_3WAY, StereoSGBM, StereoSGBM_create, createRightMatcher,
                      filterSpeckles, StereoBM, StereoBM_create)
from .settings import DEFAULT_SETTINGS, parse_config_file
from .stereo_vision import compute_disparity, matcher_from_settings
from ._lib import SmError
from .reproject import project_points_3D, reprojectImageTo3D, write_ply
from .rectify import (CALIB_ZERO_DISPARITY, COLOR_BGR2GRAY, CV_32FC1, INTER_LINEAR, StereoRectifier, cvtColor,
                      initUndistortRectifyMap, rectify_opencv, remap, stereoRectify)
from .denoise import fastNlMeansDenoising
from .pointcloud import extract_point_cloud, format_ply, write_point_cloud
from .png import (decode_disparity_png, encode_disparity_png, imdecode, imdecode_batch, imdecode_host, imencode_png,
                  imencode_png_batch, imencode_png_host, imread, imwrite, read_disparity_png, write_disparity_png)
from . import filters
from .filters import gaussian_filter, image_measure, pyrDown
from . import mccnn
from .mccnn import McCnnFast
from . import mcaccurate
from .mcaccurate import McCnnAccurate
from . import mcstereo
from .mcstereo import (McCnnCrossParams, McCnnStereo, McCnnStereoParams, mc_aggregate, mc_cross_aggregate, mc_cross_arms,
                       mc_disparity)

__all__ = [
    "compute_disparity", "matcher_from_settings", "StereoSGBM", "StereoSGBM_create", "createRightMatcher",
    "STEREO_SGBM_MODE_SGBM", "STEREO_SGBM_MODE_HH", "STEREO_SGBM_MODE_SGBM_3WAY", "STEREO_SGBM_MODE_HH4",
    "parse_config_file", "DEFAULT_SETTINGS", "SmError", "filterSpeckles", "reprojectImageTo3D",
    "project_points_3D", "write_ply", "StereoBM", "StereoBM_create",
    "stereoRectify", "initUndistortRectifyMap", "remap", "cvtColor", "rectify_opencv", "StereoRectifier",
    "CALIB_ZERO_DISPARITY", "CV_32FC1", "INTER_LINEAR", "COLOR_BGR2GRAY", "fastNlMeansDenoising",
    "extract_point_cloud", "format_ply", "write_point_cloud",
    "imwrite", "imencode_png", "imencode_png_batch", "imencode_png_host", "write_disparity_png",
    "encode_disparity_png", "imread", "imdecode", "imdecode_batch", "imdecode_host", "read_disparity_png",
    "decode_disparity_png",
    "filters", "gaussian_filter", "image_measure", "pyrDown",
    "mccnn", "McCnnFast", "mcaccurate", "McCnnAccurate",
    "mcstereo", "McCnnStereo", "McCnnStereoParams", "mc_aggregate", "mc_disparity",
    "McCnnCrossParams", "mc_cross_arms", "mc_cross_aggregate",
]
__version__ = "0.1.0"
