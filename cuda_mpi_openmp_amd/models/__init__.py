"""The workloads ("model families") of the suite, each with a single-device
form and a row/shard-decomposed multi-GPU form:

  lab1  VectorSub / ShardedVectorSub           element-wise fp64/fp32 c = a - b
  lab2  EdgeDetector / SlabEdgeDetector        Roberts cross + KxK convolutions
  lab3  PixelClassifier / SlabPixelClassifier  Mahalanobis ML classification
  lab4  DenseLU                                dense fp64 LU: solve, log-determinant, inverse (one device)
  lab4  BatchedDenseLU                         the same for a batch of small matrices, one launch each way
  lab4  DenseCholesky                          dense fp64 Cholesky of an SPD matrix: solve, log-determinant, inverse
  lab4  BatchedDenseCholesky                   the same for a batch of small SPD matrices, one launch each way
  lab4  DenseQR                                dense fp64 Householder QR (m >= n): least squares, Q, R, log|det|
  stencil  SlabJacobi                          2-D Jacobi with halo exchange
  stencil  SlabJacobi3D                        3-D Jacobi on plane slabs
  stencil  PoissonMultigrid                    2-D Poisson by geometric multigrid V-cycles (one device)
  stencil  PoissonMultigrid3D                  3-D Poisson in a box by geometric multigrid V-cycles (one device)
"""

from .classifier import PixelClassifier, SlabPixelClassifier
from .dense import BatchedDenseCholesky, BatchedDenseLU, DenseCholesky, DenseLU, DenseQR
from .edge import EdgeDetector, SlabEdgeDetector
from .jacobi import SlabJacobi
from .jacobi3d import SlabJacobi3D
from .multigrid import PoissonMultigrid
from .multigrid3d import PoissonMultigrid3D
from .vector import ShardedVectorSub, VectorSub

__all__ = ["PixelClassifier", "SlabPixelClassifier", "EdgeDetector", "SlabEdgeDetector", "SlabJacobi", "SlabJacobi3D",
           "PoissonMultigrid", "PoissonMultigrid3D", "ShardedVectorSub", "VectorSub", "DenseLU",
           "BatchedDenseLU", "DenseCholesky", "BatchedDenseCholesky", "DenseQR"]
