"""sapcu_amd — MI355X-native hot path of the SNN point-cloud upsampler.

Public surface = the reference's own interface for this path:
  ImprovedSNNNormalEstimation, EnhancedSNNDistanceEstimation  (fn/fd ``snn_coder``)
  TrainableSNNDistanceEstimation                              (fd with a training path, ``fd_train``)
  Generator3D6, SNNPointCloudGenerator                        (``generation``)
  normalize_pointcloud, farthest_point_sample, process_file   (``generate``)
  cloud_metrics, dataset_metrics, evaluate_file               (``metrics``: Chamfer, Hausdorff, F-score on the device)
  softmin, sinkhorn_potentials, sinkhorn_metrics,             (``sinkhorn``: Sinkhorn / EMD transport figures on the device, without
  dataset_sinkhorn, evaluate_sinkhorn_file                     the n x m cost matrix)
  point_to_mesh, mesh_metrics, mesh_dataset_metrics,          (``mesh``: P2F, the point-to-surface distance to a triangle mesh,
  read_off, evaluate_mesh_file                                 on the device)
  build_patches, PU1KPatches, MeshPatches,                    (``data``: fd / fn training batches from raw cloud pairs, or from
  MeshSurfacePatches                                           triangle meshes sampled afresh per batch, on the device)
  build_surface_tables, sample_surface                        (``surface``: area-weighted sampling of triangle meshes on the device)
  ray_to_mesh, signed_ray_distance, ray_metrics,              (``ray``: ray casting against triangle meshes on the device, the ground
  sample_fd_rays, as_fd_npz, is_watertight, FdRayPatches       truth of fd's directed distance, fd's ray samples from meshes)
  pca_normals, normal_angles, normal_metrics,                 (``normals``: PCA normals of a cloud and the angular error of normals
  cloud_normal_metrics, evaluate_normals_file                  on the device: fn's score, ground-truth normals, surface quality)
  geodesic_disks, disk_radii, uniformity_seeds,               (``uniformity``: how evenly a cloud covers its mesh, the NUC figures
  uniformity_metrics, dataset_uniformity, read_seeds,          of the PU-GAN protocol from exact geodesic disks on the device)
  write_seeds, evaluate_uniformity_file
  poisson_select, poisson_subsample, poisson_disk_sample,     (``poisson``: Poisson-disk selection and exact-count blue-noise
  PoissonPU1KPatches                                           subsampling of clouds and meshes on the device; fd's clouds from meshes)
  near_voxels, pointing_samples, sample_fn_pointing,          (``pointing``: fn's seed-centred samples, query points in a band off a
  as_fn_npz, seed_patches, FnPointingPatches, FdSeedPatches    surface with their pointing directions; the seed-centred loaders of fn and fd)
Importing the package never touches the GPU; the HIP library is loaded on first use and its
absence raises ``SapcuLibraryError`` (no CPU fallback exists).
"""
from ._lib import SapcuError, SapcuLibraryError, LIB_PATH  # noqa: F401
from .modules import ImprovedSNNNormalEstimation, EnhancedSNNDistanceEstimation, TrainableSNNDistanceEstimation  # noqa: F401
from .generation import Generator3D6, SNNPointCloudGenerator  # noqa: F401
from .pipeline import normalize_pointcloud, farthest_point_sample, process_cloud, process_file, evaluate_file, evaluate_sinkhorn_file  # noqa: F401
from .metrics import cloud_metrics, dataset_metrics  # noqa: F401
from .sinkhorn import softmin, sinkhorn_potentials, sinkhorn_metrics, dataset_sinkhorn  # noqa: F401
from .mesh import point_to_mesh, mesh_metrics, mesh_dataset_metrics, read_off, evaluate_mesh_file  # noqa: F401
from .data import build_patches, PU1KPatches, MeshPatches, MeshSurfacePatches, FdRayPatches, PoissonPU1KPatches  # noqa: F401
from .data import seed_patches, FnPointingPatches, FdSeedPatches  # noqa: F401
from .surface import build_surface_tables, sample_surface  # noqa: F401
from .ray import ray_to_mesh, signed_ray_distance, ray_metrics, sample_fd_rays, as_fd_npz, is_watertight  # noqa: F401
from .normals import pca_normals, normal_angles, normal_metrics, cloud_normal_metrics, evaluate_normals_file  # noqa: F401
from .uniformity import (geodesic_disks, disk_radii, uniformity_seeds, uniformity_metrics, dataset_uniformity, read_seeds,  # noqa: F401
                         write_seeds, evaluate_uniformity_file)
from .poisson import poisson_select, poisson_subsample, poisson_disk_sample  # noqa: F401
from .pointing import near_voxels, pointing_samples, sample_fn_pointing, as_fn_npz  # noqa: F401

__all__ = ["ImprovedSNNNormalEstimation", "EnhancedSNNDistanceEstimation", "TrainableSNNDistanceEstimation", "Generator3D6",
           "SNNPointCloudGenerator", "SapcuError", "SapcuLibraryError"]
