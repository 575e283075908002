// obstacle.hpp -- host mirror of the reference's obstacle / waypoint map (obstacle.hpp:13-97): boxes and ellipsoids
// read from a file, a smooth penalty around them, and the waypoint path.  Function / Gradient are evaluated on the
// host in the reference's operation order (users call the map directly; it is also the CPU-side check of the device
// table); the vtolUAV model evaluates the same penalty on the device from DeviceMapTable() / DeviceMapParams().
#ifndef SOCP_AMD_OBSTACLE_HPP_
#define SOCP_AMD_OBSTACLE_HPP_

#include <string>

#include "../../socp/map.hpp"

class obstacle : public map
{
public:
    // same members, order and types as the reference's structure (continuation writes through GetParameterData())
    struct parameters_struct {
        real phiObs;     // weight of the obstacle penalty
        real psiWP;      // weight of the waypoint penalty (multiplies zero: that part is switched off upstream)
        real muObs;      // width of the transition around an obstacle's surface
        real sigmaWP;    // width of the waypoint penalty
    };

    obstacle(std::string the_fileObstacles = std::string(""), std::string the_fileWP = std::string(""));
    obstacle(obstacle const &other);
    obstacle &operator=(obstacle const &other);
    ~obstacle() override;

    void Function(std::vector<real> const &position, real &funcTot) const override;
    void Gradient(std::vector<real> const &position, std::vector<real> &gradTot) const override;
    void ObstaclePenalizationFunction(std::vector<real> const &position, real &funcObs) const;
    void ObstaclePenalizationGradient(std::vector<real> const &position, std::vector<real> &gradObs) const;
    void WPPenalizationFunction(std::vector<real> const &position, real &funcWP) const;
    void WPPenalizationGradient(std::vector<real> const &position, std::vector<real> &gradWP) const;

    parameters_struct &GetParameterData();
    const std::vector<std::vector<real>> &GetPath();

    // device hook
    bool DeviceMapTable(std::vector<double> &table) const override;
    int DeviceMapParams(double *out, int cap) const override;

private:
    struct data_struct;
    data_struct *data;
    void ReadObstacleInput();
    void ReadWPInput();
};

#endif
