"""The two block worlds, turn based, planner (ego) and constructor (partner) -- behaviour of the reference's
pantheonrl/envs/blockworldgym (blockworld.py:34-134, simpleblockworld.py:36-234, gridutils.py:8-64).

Both games are played on a 7 x 7 grid with five two-cell blocks in two colours (1 = blue, 2 = red, 0 = none); row 0 is the
top.  A horizontal block at (y, x) covers (y, x) and (y, x + 1), a vertical one (y, x) and (y + 1, x).  The planner sees the
target and speaks one token per turn; the constructor sees the token and its own work.  The planner always moves first and
ends the game with its last token; only then is a reward paid, the same to both seats.

  * `BlockEnv` (BlockEnv-v1): the constructor drops coloured blocks from the top (gravity); the reward is the F1 score of
    the built grid against the target, 2 * matching cells / (built cells + target cells).
  * `SimpleBlockEnv` (BlockEnv-v0): the blocks lie where they are (no gravity) and the constructor only colours them;
    the reward is 100 * correctly coloured blocks / 5.

The rules are plain functions of small integer arrays, so the same statements serve the Python games, the checks of the
device kernels (csrc/ph_block.h) and the packed table state those kernels keep (`pack_state` / `unpack_state`).
"""
from __future__ import annotations

from typing import List, Sequence

import numpy as np

from ..common.agents import Agent
from ..common.multiagentenv import DummyEnv, TurnBasedEnv
from ..spaces import Discrete, MultiDiscrete

GRIDLEN = 7
NUM_BLOCKS = 5
NUM_COLORS = 2
NO_COLOR, BLUE, RED = 0, 1, 2
HORIZONTAL, VERTICAL = 0, 1
FULL_TOKENS = 30       # BlockEnv-v1
SIMPLE_TOKENS = 16     # BlockEnv-v0
STATE_WORDS = 12       # int32 words of a packed table (csrc/ph_block.h)

_CELLS = [NUM_COLORS + 1] * (GRIDLEN * GRIDLEN)
_BLOCK = [2, GRIDLEN, GRIDLEN, NUM_COLORS + 1]       # orientation, y, x, colour


def _token(action) -> int:
    """the planner's token as a plain int (a learner hands over a 0-d or one-element array)"""
    return int(np.asarray(action).reshape(-1)[0])


# ---- grid rules (BlockEnv-v1) -----------------------------------------------------------------------------------------
def gravity(grid: np.ndarray, orientation: int, x: int) -> int:
    """row at which a block dropped in column x comes to rest, -1 when its entry cells are taken"""
    n = len(grid)
    second = grid[0][x + 1] if orientation == HORIZONTAL else grid[1][x]
    if grid[0][x] != 0 or second != 0:
        return -1
    if orientation == HORIZONTAL:
        for y in range(n - 1):
            if grid[y + 1][x] != 0 or grid[y + 1][x + 1] != 0:
                return y
        return n - 1
    for y in range(n - 2):
        if grid[y + 2][x] != 0:
            return y
    return n - 2


def place(grid: np.ndarray, x: int, y: int, color: int, orientation: int) -> None:
    grid[y][x] = color
    if orientation == HORIZONTAL:
        grid[y][x + 1] = color
    else:
        grid[y + 1][x] = color


def drop_random(grid: np.ndarray, rng=np.random) -> bool:
    """one random drop (orientation, column, and -- only when it lands -- colour); False when it did not fit"""
    orientation = rng.randint(2)
    x = rng.randint(GRIDLEN - 1 if orientation == HORIZONTAL else GRIDLEN)
    y = gravity(grid, orientation, x)
    if y == -1:
        return False
    place(grid, x, y, rng.randint(NUM_COLORS) + 1, orientation)
    return True


def generate_random_world(rng=np.random) -> np.ndarray:
    grid = np.zeros((GRIDLEN, GRIDLEN))
    placed = 0
    while placed < NUM_BLOCKS:
        placed += drop_random(grid, rng)
    return grid


def matches(built: np.ndarray, target: np.ndarray) -> int:
    """cells that carry the same colour in both grids"""
    return int(np.count_nonzero((built != 0) & (built == target)))


def f1_score(built: np.ndarray, target: np.ndarray) -> float:
    return 2 * matches(built, target) / (np.count_nonzero(built) + np.count_nonzero(target))


# ---- block-list rules (BlockEnv-v0) --------------------------------------------------------------------------------------
def random_block(rng=np.random) -> List[int]:
    """draw order: orientation, x, y, colour"""
    if rng.randint(2) == 0:
        orientation, x, y = HORIZONTAL, rng.randint(GRIDLEN - 1), rng.randint(GRIDLEN)
    else:
        orientation, x, y = VERTICAL, rng.randint(GRIDLEN), rng.randint(GRIDLEN - 1)
    return [orientation, y, x, rng.randint(NUM_COLORS) + 1]


def block_cells(block: Sequence[int]):
    o, y, x = int(block[0]), int(block[1]), int(block[2])
    return ((y, x), (y, x + 1)) if o == HORIZONTAL else ((y, x), (y + 1, x))


def generate_block_list(rng=np.random) -> List[List[int]]:
    """five random blocks that do not overlap; a block that does is drawn again"""
    taken, blocks = set(), []
    while len(blocks) < NUM_BLOCKS:
        block = random_block(rng)
        cells = block_cells(block)
        if cells[0] in taken or cells[1] in taken:
            continue
        taken.update(cells)
        blocks.append(block)
    return blocks


# ---- packed table state of the device kernels -------------------------------------------------------------------------
def _pack_grid(grid: np.ndarray) -> List[int]:
    """49 two-bit cells, row major, 16 per 32-bit word"""
    words = [0, 0, 0, 0]
    for k, v in enumerate(np.asarray(grid).reshape(-1)):
        words[k >> 4] |= (int(v) & 3) << (2 * (k & 15))
    return words


def _unpack_grid(words: Sequence[int]) -> np.ndarray:
    cells = [(int(words[k >> 4]) >> (2 * (k & 15))) & 3 for k in range(GRIDLEN * GRIDLEN)]
    return np.array(cells, np.int64).reshape(GRIDLEN, GRIDLEN)


def pack_state(variant: int, world, view=None, token: int = 0) -> np.ndarray:
    """(12,) int32 table state.  variant 1: world / view are the target / built grids (7, 7); variant 0: world is the block
    list (5, 4) and view the constructor's colours (5,), all none by default."""
    w = np.zeros(STATE_WORDS, np.int64)
    if variant == 1:
        w[0:4] = _pack_grid(world)
        w[4:8] = _pack_grid(np.zeros((GRIDLEN, GRIDLEN)) if view is None else view)
    else:
        for i, (o, y, x, c) in enumerate(np.asarray(world, np.int64)):
            w[i] = int(o) | int(y) << 1 | int(x) << 4 | int(c) << 7
        colours = [0] * NUM_BLOCKS if view is None else view
        w[5] = sum((int(c) & 3) << (2 * i) for i, c in enumerate(colours))
    w[8] = int(token)
    return (w & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def unpack_state(variant: int, state):
    """-> (world, view, token), the arguments of `pack_state`"""
    w = np.asarray(state, np.int32).view(np.uint32).astype(np.int64)
    if variant == 1:
        return _unpack_grid(w[0:4]), _unpack_grid(w[4:8]), int(w[8])
    blocks = np.array([[w[i] & 1, (w[i] >> 1) & 7, (w[i] >> 4) & 7, (w[i] >> 7) & 3] for i in range(NUM_BLOCKS)], np.int64)
    colours = np.array([(w[5] >> (2 * i)) & 3 for i in range(NUM_BLOCKS)], np.int64)
    return blocks, colours, int(w[8])


# ---- BlockEnv-v1 --------------------------------------------------------------------------------------------------------
class BlockEnv(TurnBasedEnv):
    observation_space = MultiDiscrete(_CELLS + _CELLS)                     # planner: target grid, built grid
    action_space = Discrete(FULL_TOKENS)
    partner_observation_space = MultiDiscrete([FULL_TOKENS] + _CELLS)     # constructor: last token, built grid
    partner_action_space = MultiDiscrete([GRIDLEN, 2, NUM_COLORS])        # x, orientation, colour - 1
    partner_env = DummyEnv(partner_observation_space, partner_action_space)
    END_TOKEN = FULL_TOKENS - 1

    def __init__(self):
        super().__init__(probegostart=1)
        self.gridworld = np.zeros((GRIDLEN, GRIDLEN))
        self.constructor_obs = np.zeros((GRIDLEN, GRIDLEN))
        self.last_token = 0

    def getDummyEnv(self, player_num: int):
        return self.partner_env if player_num else self

    def multi_reset(self, egofirst: bool):
        self.gridworld = generate_random_world()
        self.constructor_obs = np.zeros((GRIDLEN, GRIDLEN))
        self.last_token = 0
        return self.get_obs(egofirst)

    def get_obs(self, isego: bool) -> np.ndarray:
        if isego:
            return np.concatenate((self.gridworld, self.constructor_obs), axis=None)
        return np.array([self.last_token] + list(self.constructor_obs.flatten()))

    def get_reward(self) -> float:
        return f1_score(self.constructor_obs, self.gridworld)

    def ego_step(self, action):
        self.last_token = _token(action)
        done = self.last_token == self.END_TOKEN
        reward = self.get_reward() if done else 0
        return self.get_obs(False), [reward, reward], done, {}

    def alt_step(self, action):
        x, orientation, color = int(action[0]), int(action[1]), int(action[2]) + 1
        if not (orientation == HORIZONTAL and x == GRIDLEN - 1):
            y = gravity(self.constructor_obs, orientation, x)
            if y != -1:
                place(self.constructor_obs, x, y, color, orientation)
        return self.get_obs(True), [0, 0], False, {}


class DefaultConstructorAgent(Agent):
    """reads a token as (column, orientation, colour): token - 1 = 4 * x + 2 * orientation + colour; the first and the last
    token ask for nothing in particular and get a blue vertical block in the last column"""

    def get_action(self, obs, record=True):
        token = int(obs.obs[0])
        if token == 0 or token == FULL_TOKENS - 1:
            return [GRIDLEN - 1, VERTICAL, 0]
        t = token - 1
        return [t // 4, (t // 2) % 2, t % 2]

    def update(self, reward, done):
        return None


# ---- BlockEnv-v0 --------------------------------------------------------------------------------------------------------
class SimpleBlockEnv(TurnBasedEnv):
    observation_space = MultiDiscrete(_BLOCK * NUM_BLOCKS + _BLOCK * NUM_BLOCKS)     # planner: true blocks, constructor's view
    action_space = Discrete(SIMPLE_TOKENS)
    partner_observation_space = MultiDiscrete([SIMPLE_TOKENS] + _BLOCK * NUM_BLOCKS)
    partner_action_space = MultiDiscrete([NUM_BLOCKS, NUM_COLORS + 1])               # block index, colour
    partner_env = DummyEnv(partner_observation_space, partner_action_space)
    END_TOKEN = SIMPLE_TOKENS - 1

    def __init__(self):
        super().__init__(probegostart=1)
        self.gridworld: List[List[int]] = [[0, 0, 0, 0] for _ in range(NUM_BLOCKS)]
        self.constructor_obs: List[List[int]] = [[0, 0, 0, 0] for _ in range(NUM_BLOCKS)]
        self.last_token = 0

    def getDummyEnv(self, player_num: int):
        return self.partner_env if player_num else self

    def multi_reset(self, egofirst: bool):
        self.gridworld = generate_block_list()
        self.constructor_obs = [[b[0], b[1], b[2], NO_COLOR] for b in self.gridworld]
        self.last_token = 0
        return self.get_obs(egofirst)

    def get_obs(self, isego: bool) -> np.ndarray:
        if isego:
            return np.array([self.gridworld, self.constructor_obs]).flatten()
        return np.array([self.last_token] + [v for block in self.constructor_obs for v in block])

    def get_reward(self) -> List[float]:
        correct = sum(1 for true, seen in zip(self.gridworld, self.constructor_obs) if true[3] == seen[3])
        reward = 100 * correct / NUM_BLOCKS
        return [reward, reward]

    def ego_step(self, action):
        self.last_token = _token(action)
        done = self.last_token == self.END_TOKEN
        return self.get_obs(False), (self.get_reward() if done else [0, 0]), done, {}

    def alt_step(self, action):
        self.constructor_obs[int(action[0])][3] = int(action[1])     # (a negative index counts from the last block, as a list does)
        return self.get_obs(True), [0, 0], False, {}


def _pass_move(obs):
    """the move that changes nothing: give block 0 the colour it already has"""
    return [0, obs[4]]


class SBWEasyPartner(Agent):
    """tokens 1-5 colour block token - 1 red, 6-10 colour block token - 8 blue (so 6 and 7 reach the last two blocks from
    behind); tokens above 10 are halved first"""

    def get_action(self, obs, record=True):
        obs = obs.obs
        token = obs[0]
        if token > 10:
            token = token // 2
        if 1 <= token <= 5:
            return [token - 1, RED]
        if 6 <= token <= 10:
            return [token - 8, BLUE]
        return _pass_move(obs)

    def update(self, reward, done):
        return None


class SBWDefaultAgent(Agent):
    """tokens 1-7 / 8-14 name a grid row: colour the first still uncoloured block met along it red / blue"""

    def get_action(self, obs, record=True):
        obs = obs.obs
        token = obs[0]
        if token == 0:
            return _pass_move(obs)
        blocks = np.reshape(obs[1:], (NUM_BLOCKS, 4))
        owner = self.owners(blocks)
        if token <= 7:
            index = self.first_uncoloured(owner, token - 1, blocks)
            if index != -1:
                return [index, RED]
        if token <= 14:
            index = self.first_uncoloured(owner, token - 8, blocks)     # (a red-range token whose row is done looks again
            if index != -1:                                             #  at row token - 8 < 0, counted from the bottom)
                return [index, BLUE]
        return _pass_move(obs)

    @staticmethod
    def first_uncoloured(owner, row, blocks):
        for index in owner[row]:
            if index != -1 and blocks[index][3] == NO_COLOR:
                return index
        return -1

    @staticmethod
    def owners(blocks) -> np.ndarray:
        """(7, 7) index of the block covering each cell, -1 where none does"""
        owner = np.full((GRIDLEN, GRIDLEN), -1)
        for i, block in enumerate(blocks):
            for y, x in block_cells(block):
                owner[y][x] = i
        return owner

    def update(self, reward, done):
        return None
