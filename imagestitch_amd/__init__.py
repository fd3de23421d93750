"""imagestitch_amd — MI355X-native warp + multi-band blend hot path of mhhai/ImageStitch.

The package is a thin host-side mirror of the reference's call surface
(cv::detail::RotationWarper / cv::detail::Blender) over the C-ABI HIP library
imagestitch_amd/csrc/libimagestitch_hip.so (include/imagestitch_hip.h).  No CPU fallback exists.
"""
from ._lib import (BORDER_CONSTANT, BORDER_REFLECT, BORDER_REFLECT_101, BORDER_REPLICATE, INTER_LINEAR,  # noqa: F401
                   INTER_NEAREST, INTER_TIES_EVEN, PREC_F16ACC32, PREC_F32, PREC_I16, IsxError, load)
from .blender import Blender, FeatherBlender, MultiBandBlender, NoBlender, convert_to, dilate_and, gain_apply  # noqa: F401
from .cameras import CameraParams, HomographyBasedEstimator, estimate_cameras  # noqa: F401
from .adjuster import (WAVE_CORRECT_HORIZ, WAVE_CORRECT_VERT, BundleAdjusterRay, BundleAdjusterReproj, bundle_adjust_ray,  # noqa: F401
                       bundle_adjust_reproj, wave_correct, waveCorrect)
from .exposure import BlocksGainCompensator, GainCompensator  # noqa: F401
from .imgio import imread, imwrite  # noqa: F401
from .features import ImageFeatures, OrbFeaturesFinder, orb_find, SurfFeaturesFinder, SurfParams, surf_find, surf_reserve  # noqa: F401
from .features import SiftFeaturesFinder, SiftParams, sift_find, sift_reserve  # noqa: F401
from .homography import BestOf2NearestMatcher, find_homography  # noqa: F401
from .matcher import FeaturesMatcher, MatchesInfo  # noqa: F401
from .resize import dilate_resize_and, resize  # noqa: F401
from .seam import DP_COLOR, DP_COLOR_GRAD, DpSeamFinder, GraphCutSeamFinder, VoronoiSeamFinder, seam_estimate, seam_gradients  # noqa: F401
from ._lib import WARP_CYLINDRICAL, WARP_FISHEYE, WARP_PLANE, WARP_SPHERICAL, WARP_STEREOGRAPHIC  # noqa: F401
from .warper import (CylindricalWarper, FisheyeWarper, PlaneWarper, RotationWarper, SphericalWarper, StereographicWarper,  # noqa: F401
                     remap)

__all__ = ["Blender", "MultiBandBlender", "FeatherBlender", "NoBlender", "convert_to", "dilate_and", "gain_apply", "GainCompensator", "BlocksGainCompensator", "imread", "imwrite", "resize", "dilate_resize_and", "INTER_NEAREST", "INTER_LINEAR", "seam_estimate", "seam_gradients", "DP_COLOR", "DP_COLOR_GRAD", "DpSeamFinder", "GraphCutSeamFinder", "VoronoiSeamFinder", "OrbFeaturesFinder", "ImageFeatures", "orb_find", "SurfFeaturesFinder", "SurfParams", "surf_find", "surf_reserve", "SiftFeaturesFinder", "SiftParams", "sift_find", "sift_reserve", "FeaturesMatcher", "BestOf2NearestMatcher", "MatchesInfo", "find_homography", "CameraParams", "HomographyBasedEstimator", "estimate_cameras", "BundleAdjusterRay", "bundle_adjust_ray", "BundleAdjusterReproj", "bundle_adjust_reproj", "wave_correct", "waveCorrect", "WAVE_CORRECT_HORIZ", "WAVE_CORRECT_VERT", "remap", "CylindricalWarper", "SphericalWarper", "PlaneWarper", "FisheyeWarper", "StereographicWarper", "WARP_CYLINDRICAL", "WARP_SPHERICAL", "WARP_PLANE", "WARP_FISHEYE", "WARP_STEREOGRAPHIC", "RotationWarper", "IsxError", "load"]
