from ..models.regression import (DecisionTreeRegressionModel, DecisionTreeRegressor, FMRegressionModel,  # noqa: F401
                                 FMRegressor, GBTRegressionModel,
                                 GBTRegressor, GeneralizedLinearRegression, GeneralizedLinearRegressionModel,
                                 GeneralizedLinearRegressionSummary, GeneralizedLinearRegressionTrainingSummary,
                                 IsotonicRegression, IsotonicRegressionModel, LinearRegression,
                                 LinearRegressionModel, RandomForestRegressionModel, RandomForestRegressor)
