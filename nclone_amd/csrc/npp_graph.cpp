// npp_graph.cpp -- host-side builder of the per-level graph observation tables (npp_graph.hpp) and the host-only C entry point
// for the CPU test-suite.  The adjacency is the reachability builder's (build_adjacency, npp_reach.cpp); this file restates
// what the reference does with it (graph/edge_building.py:124-272, graph/feature_builder.py:67-197).
#include "npp_graph.hpp"

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/npp_amd.h"
#include "npp_level.hpp"
#include "npp_reach_build.hpp"
#include "npp_reach_features.hpp"

namespace npp {
namespace {

const int DX[8] = {0, 1, 0, -1, 1, 1, -1, -1}, DY[8] = {-1, 0, 1, 0, -1, 1, 1, -1};   // N E S W NE SE SW NW

// one entry of level_data.entities that can give a node entity info, with features 2-5 it gives
struct GraphEnt {
    double x, y;
    float f[4];
};

// entity_extractor.py:37-270 in its order, at the spawn state (the ninja comes first but is of no type that counts)
std::vector<GraphEnt> graph_entities(const CompiledLevel &L) {
    std::vector<int> switches, doors, locked, mines1, mines21;
    for (size_t k = 0; k < L.ent_map_order.size(); k++) {
        const int s = L.ent_map_order[k];
        const uint32_t kind = L.ent_meta[s] & 15u, type = (L.ent_meta[s] >> 24) & 63u;
        if (kind == EK_SWITCH) switches.push_back(s);
        else if (kind == EK_EXIT) doors.push_back(s);
        else if (kind == EK_LOCKED) locked.push_back(s);
        else if (kind == EK_MINE) (type == 1 ? mines1 : mines21).push_back(s);
    }
    std::vector<GraphEnt> out;
    // exit switch i, then exit door i when there is one (_extract_exit_entities); both active at the spawn
    for (size_t i = 0; i < switches.size(); i++) {
        out.push_back({L.ent_x[switches[i]], L.ent_y[switches[i]], {0.f, 0.f, 1.f, 0.f}});
        if (i < doors.size()) out.push_back({L.ent_x[doors[i]], L.ent_y[doors[i]], {0.f, 0.f, 1.f, 0.f}});
    }
    // locked doors (_extract_locked_doors): the switch part at the entity, the door part at the midpoint of its segment; active and
    // closed at the spawn
    for (int s : locked) {
        out.push_back({L.ent_x[s], L.ent_y[s], {0.f, 0.f, 1.f, 1.f}});
        double dx = 0.0, dy = 0.0;
        for (size_t d = 0; d + 4 < L.door_segs.size(); d += 5)
            if ((int)L.door_segs[d + 4] == s) {
                dx = (L.door_segs[d] + L.door_segs[d + 2]) * 0.5;
                dy = (L.door_segs[d + 1] + L.door_segs[d + 3]) * 0.5;
                break;
            }
        out.push_back({dx, dy, {0.f, 0.f, 1.f, 1.f}});
    }
    // toggle mines (_extract_mines): type 1 in its state at the spawn, type 21 always state 0; mine state -1 deadly (0),
    // 0 toggling (2), +1 safe (1); radius TOGGLE_MINE_RADII[state] / (2 * NINJA_RADIUS)
    static const double RADII[3] = {4.0, 3.5, 4.5};
    auto mine = [&](int s, uint32_t state) {
        const float ms = state == 0 ? -1.f : (state == 2 ? 0.f : 1.f);
        double r = RADII[state < 3 ? state : 1] / 20.0;
        r = r < 0.0 ? 0.0 : (r > 1.0 ? 1.0 : r);
        out.push_back({L.ent_x[s], L.ent_y[s], {ms, (float)r, 1.f, 0.f}});
    };
    for (int s : mines1) mine(s, (L.ent_meta[s] >> 4) & 3u);
    for (int s : mines21) mine(s, 0u);
    return out;
}

void node_features(int x, int y, const std::vector<GraphEnt> &ents, float *f) {
    double fx = (double)x / 1056.0, fy = (double)y / 600.0;   // LEVEL_WIDTH_PX, LEVEL_HEIGHT_PX
    f[0] = (float)(fx < 0.0 ? 0.0 : (fx > 1.0 ? 1.0 : fx));
    f[1] = (float)(fy < 0.0 ? 0.0 : (fy > 1.0 ? 1.0 : fy));
    f[2] = f[3] = f[4] = f[5] = 0.f;
    for (const GraphEnt &e : ents)   // get_entities_in_region: inclusive box of half-width TILE_PIXEL_SIZE // 2
        if (x - 12 <= e.x && e.x <= x + 12 && y - 12 <= e.y && e.y <= y + 12) {
            std::memcpy(f + 2, e.f, sizeof(e.f));
            return;
        }
}

}  // namespace

void build_graph_obs(const CompiledLevel &L, GraphBuilt &G) {
    ReachAdjacency A;
    build_adjacency(L, A);
    // nodes: every endpoint of an edge, in (x, y) order = ascending node id (x = 6 + 12 i, y = 6 + 12 j, id = i * RH + j)
    std::vector<uint8_t> node(RNODES, 0);
    for (int id = 0; id < RNODES; id++)
        for (int d = 0; d < 8; d++)
            if ((A.adj[id] >> d) & 1u) {
                node[id] = 1;
                node[(id / RH + DX[d]) * RH + id % RH + DY[d]] = 1;
            }
    std::vector<int32_t> idx(RNODES, -1);
    std::vector<int> ids;
    for (int id = 0; id < RNODES; id++)
        if (node[id]) { idx[id] = (int32_t)ids.size(); ids.push_back(id); }
    const std::vector<GraphEnt> ents = graph_entities(L);
    G = GraphBuilt();
    if (ids.empty()) {   // "If no positions, create at least one node": (0, 0)
        G.n_nodes = 1;
        G.feats.resize(GRAPH_FEAT);
        node_features(0, 0, ents, G.feats.data());
        return;
    }
    G.n_nodes = (uint32_t)std::min<size_t>(ids.size(), GRAPH_NODES);
    G.feats.resize((size_t)G.n_nodes * GRAPH_FEAT);
    for (uint32_t k = 0; k < G.n_nodes; k++) node_features(reach_node_x(ids[k]), reach_node_y(ids[k]), ents, &G.feats[(size_t)k * GRAPH_FEAT]);
    // edges in the adjacency dict's order; those touching a truncated node are skipped
    std::vector<int> src(RNODES);
    for (int id = 0; id < RNODES; id++) src[id] = id;
    std::sort(src.begin(), src.end(), [](int a, int b) { return reach_order_key(a) < reach_order_key(b); });
    std::vector<uint16_t> s, t;
    for (int id : src) {
        if (!A.in[id]) continue;
        for (int d = 0; d < 8 && s.size() < (size_t)GRAPH_EDGES; d++) {
            if (!((A.adj[id] >> d) & 1u)) continue;
            const int nb = (id / RH + DX[d]) * RH + id % RH + DY[d];
            if (idx[id] >= GRAPH_NODES || idx[nb] >= GRAPH_NODES) continue;
            s.push_back((uint16_t)idx[id]);
            t.push_back((uint16_t)idx[nb]);
        }
    }
    G.n_edges = (uint32_t)s.size();
    G.edges = s;
    G.edges.insert(G.edges.end(), t.begin(), t.end());
}

void pack_graph_obs(const GraphBuilt &G, GraphHdr &hdr, std::vector<unsigned char> &blob) {
    auto append = [&](const void *p, size_t bytes) -> uint64_t {
        const size_t off = (blob.size() + 15) / 16 * 16;
        blob.resize(off + (bytes + 15) / 16 * 16, 0);
        if (bytes) std::memcpy(blob.data() + off, p, bytes);
        return (uint64_t)off;
    };
    hdr.n_nodes = G.n_nodes;
    hdr.n_edges = G.n_edges;
    hdr.off_feats = append(G.feats.data(), 4 * G.feats.size());
    hdr.off_src = append(G.edges.data(), 2 * (size_t)G.n_edges);
    hdr.off_dst = append(G.edges.data() + G.n_edges, 2 * (size_t)G.n_edges);
}

}  // namespace npp

using namespace npp;

extern "C" {

int npp_graph_compile(const double *map, int64_t n, float *feats, uint16_t *edge_index, int32_t *counts) {
    if (!map) return NPP_ERR_INVALID;
    CompiledLevel L;
    std::string err;
    if (!compile_level(map, n, L, err)) return NPP_ERR_INVALID;
    GraphBuilt G;
    build_graph_obs(L, G);
    if (feats) {
        std::memset(feats, 0, GRAPH_FEAT_ROW);
        std::memcpy(feats, G.feats.data(), 4 * G.feats.size());
    }
    if (edge_index) {
        std::memset(edge_index, 0, GRAPH_EDGE_ROW);
        std::memcpy(edge_index, G.edges.data(), 2 * (size_t)G.n_edges);
        std::memcpy(edge_index + GRAPH_EDGES, G.edges.data() + G.n_edges, 2 * (size_t)G.n_edges);
    }
    if (counts) { counts[0] = (int32_t)G.n_nodes; counts[1] = (int32_t)G.n_edges; }
    return NPP_OK;
}

}  // extern "C"
