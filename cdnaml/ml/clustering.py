from ..models.clustering import (BisectingKMeans, GaussianMixture, GaussianMixtureModel,  # noqa: F401
                                 GaussianMixtureSummary, KMeans, KMeansModel, KMeansSummary, MultivariateGaussian)
