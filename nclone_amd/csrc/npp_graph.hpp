// npp_graph.hpp -- graph observations for the GCN encoder (graph_node_feats / graph_edge_index / graph_node_mask /
// graph_edge_mask): data model shared by the host builder (npp_graph.cpp), the C ABI and the kernel (npp_graph.hip).
//
// What the reference computes (citations: files of its nclone package):
//   gym_environment/mixins/graph_mixin.py:96-109, 340-376   at every reset, from the freshly loaded level: build_graph from the
//                                                           spawn, then the GraphData; within an episode it never changes (the
//                                                           map-name cache hit returns before current_graph is touched)
//   gym_environment/mixins/graph_mixin.py:587-605           edges = the `adjacency` dict as it iterates: sources in dict order,
//                                                           neighbours N E S W NE SE SW NW
//   graph/edge_building.py:124-272 create_graph_data        nodes = endpoints of edges, sorted by (x, y), at most N_MAX_NODES;
//                                                           no edge at all -> one node at (0, 0); edges touching a truncated node
//                                                           skipped, at most E_MAX_EDGES
//   graph/edge_building.py:17-66 _extract_entity_info       the first entity of level_data.entities (entity_extractor.py:37-270
//                                                           order: ninja, exit switch / door pairs, locked doors as switch part
//                                                           then door part, toggle mines type 1, then type 21) inside
//                                                           [x - 12, x + 12] x [y - 12, y + 12] (level_data.py:313) -- node
//                                                           positions in tile-data space, entity positions in world space, as the
//                                                           reference compares them
//   graph/feature_builder.py:67-197                         x / 1056, y / 600; mine state and radius / 20; active; closed
// Everything is a function of the level alone: the host builds a compact table per level, the device expands it into the
// reference's dense per-env rows for the envs whose level differs from the level their rows hold.
#pragma once
#include <cstdint>
#include <vector>

namespace npp {

constexpr int GRAPH_NODES = 2500;    // N_MAX_NODES (graph/common.py:42)
constexpr int GRAPH_EDGES = 20000;   // E_MAX_EDGES (graph/common.py:48)
constexpr int GRAPH_FEAT = 6;        // NODE_FEATURE_DIM (graph/common.py:58)
// bytes of one env's row in each output
constexpr uint32_t GRAPH_FEAT_ROW = GRAPH_NODES * GRAPH_FEAT * 4;   // 60 000
constexpr uint32_t GRAPH_EDGE_ROW = 2 * GRAPH_EDGES * 2;            // 80 000 (source row, then target row)
constexpr uint32_t GRAPH_NMASK_ROW = GRAPH_NODES;                   // 2 500
constexpr uint32_t GRAPH_EMASK_ROW = GRAPH_EDGES;                   // 20 000

// Per-level table in HBM: offsets in bytes into the blob of all levels, every section 16-byte aligned and zero-padded to a
// multiple of 16 bytes (the kernel copies whole 16-byte words and the padding is the start of the row's zero tail).
struct GraphHdr {
    uint64_t off_feats;   // f32 [n_nodes][6]
    uint64_t off_src;     // u16 [n_edges]
    uint64_t off_dst;     // u16 [n_edges]
    uint32_t n_nodes, n_edges;
};

// host side (npp_graph.cpp): the compact table of one level
struct CompiledLevel;
struct GraphBuilt {
    uint32_t n_nodes = 0, n_edges = 0;
    std::vector<float> feats;      // [n_nodes][6]
    std::vector<uint16_t> edges;   // [2][n_edges]: sources, then targets
};
void build_graph_obs(const CompiledLevel &level, GraphBuilt &out);
// appends the level's table to `blob` (16-byte aligned sections), offsets in `hdr`
void pack_graph_obs(const GraphBuilt &G, GraphHdr &hdr, std::vector<unsigned char> &blob);

}  // namespace npp
