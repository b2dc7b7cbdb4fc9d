from ..models.clustering import (BisectingKMeans, BisectingKMeansModel, BisectingKMeansSummary,  # noqa: F401
                                 GaussianMixture, GaussianMixtureModel, GaussianMixtureSummary, KMeans, KMeansModel,
                                 KMeansSummary, MultivariateGaussian)
